/*
 * grid_capi.h - C ABI of a robot-specialised GRiD library for AMD MI355X (gfx950).
 *
 * One shared library is built per robot (libgrid_<robot>.so) from the header emitted by
 * gridcodegenerator_amd.GRiDCodeGenerator(robot).gen_all_code() plus gridcodegenerator_amd/csrc/grid_capi.hip.
 * The entry points below are what a foreign-function binding (ctypes, cgo, JNI ...) of the reference's emitted
 * C++ host API would bind; each cites the reference interface it replaces.  Plain pointers and sizes only.
 *
 * Conventions
 *   - every function returns 0 on success or a non-zero hipError_t value; grid_last_error() gives the text (per calling thread).
 *     No entry point ever exit()s or aborts the host process: the reference's host API prints "GPUassert: ..." and exit()s
 *     (reference GRiDCodeGenerator.py:279-286); the shim re-binds the generated header's error hook (GRID_ON_GPU_ERROR) instead;
 *   - T is float ("Suggested Type T is float", reference GRiDCodeGenerator.py:378); every entry point also exists as *_f64
 *     (the T = double instantiation of the same generated kernels; its buffers are allocated by the first *_f64 call);
 *   - layouts (reference algorithms/_forward_dynamics_gradient.py:50,61,168 and SURVEY.md section 8(a) a1):
 *       q_qd_u [k*stride + {0..n | n..2n | 2n..3n}]            inputs, array-of-structs over the batch index k
 *       df_du  [k*2n^2 + col*n + row], col in [0,2n)           = [d qdd/d q | d qdd/d qd], column-major n x 2n
 *       dc_du  same shape as df_du;  Minv [k*n^2 + col*n + row] (upper triangle, column-major);  c, qdd [k*n + i]
 *   - gravity is passed POSITIVE (9.81), as in the reference's emitted code (reference _inverse_dynamics.py:123);
 *   - *_device entry points take DEVICE pointers and enqueue on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) without synchronising; *_host entry points take HOST pointers, copy in, run, copy out and synchronise.
 *   - one handle per GPU.  Every entry point makes the handle's device current for the duration of the call and restores the
 *     caller's device afterwards, so one process may hold a handle per GPU and call them in any order from any thread;
 *     a single handle is not thread-safe.  grid_forward_dynamics_gradient_multi_host drives G handles at once.
 */
#ifndef GRID_CAPI_H
#define GRID_CAPI_H

#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct grid_handle grid_handle;

/* robot the library was generated for (constants NUM_JOINTS etc., reference GRiDCodeGenerator.py:94-111) */
int grid_num_joints(void);
const char *grid_robot_name(void);
int grid_lanes_per_solve(void);
int grid_suggested_threads(void);
int grid_lds_bytes_per_block(void);
int grid_has_second_order(void); /* 1 if idsva_so / fdsva_so are emitted for this robot (GRID_HAS_IDSVA_SO of the generated header) */
const char *grid_last_error(void);

/* replaces init_robotModel<T>() + init_grid<T>() + init_gridData<T>(max_timesteps)
 * (reference helpers/_topology_helpers.py:715-730, GRiDCodeGenerator.py:160-271) */
int grid_init(int device, int max_timesteps, grid_handle **out);
/* replaces close_grid<T>() (reference GRiDCodeGenerator.py:252-271) */
int grid_close(grid_handle *h);
/* device the handle was created on (-1 for NULL) */
int grid_device(const grid_handle *h);
/* Page-locked host buffers (hipHostMalloc / hipHostFree).  Replaces the pinned h_* members of gridData that the reference's callers fill and read
 * (reference GRiDCodeGenerator.py:160-213 allocates them with malloc; ours with hipHostMalloc).  grid_forward_dynamics_gradient_host overlaps its
 * copies with the kernel when BOTH of its buffers come from here (or are otherwise page-locked); pageable buffers take the sequential form. */
int grid_set_host_chunks(grid_handle *h, int chunks); /* chunks of the pipelined host entry point; 0 = automatic (tuning aid, like grid_set_launch_dims) */
int grid_host_alloc(size_t bytes, void **out);
int grid_host_free(void *p);
/* solves per call the second-order entry points accept on this handle: min(max_timesteps, 1 GiB / record) - the generated init_gridData<T>()
 * caps the d_idsva_so / d_df2 buffers (4 n^3 values per solve; grid_so_max_timesteps<T>() of the generated header).  f64 != 0: the _f64 forms */
int grid_second_order_capacity(const grid_handle *h, int f64);

/* replaces forward_dynamics_gradient<T,false>(hd_data, d_robotModel, gravity, num_timesteps, block, thread, streams)
 * (reference algorithms/_forward_dynamics_gradient.py:186-249): host buffers in, host buffers out, synchronous */
int grid_forward_dynamics_gradient_host(grid_handle *h, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_df_du);
/* replaces forward_dynamics_gradient_compute_only<T,false> / a direct forward_dynamics_gradient_kernel<T> launch
 * (reference algorithms/_forward_dynamics_gradient.py:113-184,203-234): device buffers, asynchronous on `stream` */
int grid_forward_dynamics_gradient_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, int num_timesteps, float gravity,
                                          float *d_df_du, void *stream);
/* the (q,qd,qdd,Minv)-input overload, USE_QDD_MINV_FLAG=true (reference :126-130,160,233) */
int grid_forward_dynamics_gradient_qdd_minv_device(grid_handle *h, const float *d_q_qd, int stride_q_qd, const float *d_qdd, const float *d_Minv,
                                                   int num_timesteps, float gravity, float *d_df_du, void *stream);
/* launch geometry override for the *_device entry points (0 = library default).  The reference API takes
 * block_dimms/thread_dimms from the caller on every call (reference :198-199). */
int grid_set_launch_dims(grid_handle *h, int blocks, int threads);

/* SURVEY.md section 8(f) "next" rows: the stand-alone algorithms the hot path is composed of */
/* replaces inverse_dynamics_kernel<T> (reference algorithms/_inverse_dynamics.py:371-438); d_qdd may be NULL (qdd = 0) */
int grid_inverse_dynamics_device(grid_handle *h, const float *d_q_qd, int stride_q_qd, const float *d_qdd, int num_timesteps, float gravity,
                                 float *d_c, void *stream);
/* replaces direct_minv_kernel<T> (reference algorithms/_direct_minv.py:478-525) */
int grid_direct_minv_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_Minv, void *stream);
/* replaces forward_dynamics_kernel<T> (reference algorithms/_forward_dynamics.py:149-199) */
int grid_forward_dynamics_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, int num_timesteps, float gravity, float *d_qdd, void *stream);
/* replaces aba_kernel<T> (reference algorithms/_aba.py:482-537): O(n) articulated-body forward dynamics, same result as grid_forward_dynamics_device */
int grid_aba_device(grid_handle *h, const float *d_q_qd_tau, int stride_q_qd, int num_timesteps, float gravity, float *d_qdd, void *stream);
/* replaces idsva_so_kernel<T> (reference algorithms/_idsva_so.py:958-1028): second-order derivatives of inverse dynamics, 4 n^3 values per solve
 * [d2tau_dq2 | d2tau_dqd2 | d2tau_dvdq | dM_dq]; d_qdd may be NULL (qdd = 0).  Robots without the second-order kernels (grid_has_second_order() == 0) return hipErrorNotSupported;
 * launches with at most IDSVA_SO_SUGGESTED_THREADS threads per block whatever grid_set_launch_dims() says */
int grid_idsva_so_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, const float *d_qdd, int num_timesteps, float gravity,
                         float *d_idsva_so, void *stream);
/* replaces fdsva_so_kernel<T> (reference algorithms/_fdsva_so.py:159-230): second-order derivatives of forward dynamics, 4 n^3 values per solve
 * [d2a_dqdq | d2a_dvdv | d2a_dvdq | d2a_dtdq].  hipErrorNotSupported when grid_has_second_order() == 0; launches with at most
 * FDSVA_SO_SUGGESTED_THREADS threads per block whatever grid_set_launch_dims() says.  Robots whose 4 n^3 record is larger than the LDS of a
 * CU (30 joints: 432 KB; GRID_SO_DIRECT of the generated header) keep the idsva_so tensors in the handle's own workspace: num_timesteps must
 * not exceed grid_second_order_capacity() and calls on one handle must not overlap */
int grid_fdsva_so_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, int num_timesteps, float gravity, float *d_df2, void *stream);
/* replaces inverse_dynamics_gradient_kernel<T> (reference algorithms/_inverse_dynamics_gradient.py:817-888); d_qdd may be NULL */
int grid_inverse_dynamics_gradient_device(grid_handle *h, const float *d_q_qd, int stride_q_qd, const float *d_qdd, int num_timesteps, float gravity,
                                          float *d_dc_du, void *stream);

/* Host-buffer forms of the stand-alone algorithms: H2D, launch, D2H, synchronous - the semantics of the reference's host wrappers
 * inverse_dynamics<T,USE_QDD_FLAG,USE_COMPRESSED_MEM> (reference algorithms/_inverse_dynamics.py:440-512: stride 2n = compressed, 3n = q_qd_u; NULL h_qdd =
 * USE_QDD_FLAG false), inverse_dynamics_gradient<T,...> (_inverse_dynamics_gradient.py:890-962), direct_minv<T,USE_COMPRESSED_MEM> (_direct_minv.py:527-588:
 * stride n or 3n), forward_dynamics<T> (_forward_dynamics.py:199-265), aba<T> (_aba.py:539-600), idsva_so_host<T,USE_QDD_FLAG> (_idsva_so.py:1030-1090),
 * fdsva_so<T> (_fdsva_so.py:246-316), forward_dynamics_gradient<T,true> (_forward_dynamics_gradient.py:186-249).  num_timesteps <= grid_init's max_timesteps. */
int grid_inverse_dynamics_host(grid_handle *h, const float *h_q_qd, int stride_q_qd, const float *h_qdd, int num_timesteps, float gravity, float *h_c);
int grid_inverse_dynamics_gradient_host(grid_handle *h, const float *h_q_qd, int stride_q_qd, const float *h_qdd, int num_timesteps, float gravity, float *h_dc_du);
int grid_direct_minv_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_Minv);
int grid_forward_dynamics_host(grid_handle *h, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_qdd);
int grid_aba_host(grid_handle *h, const float *h_q_qd_tau, int num_timesteps, float gravity, float *h_qdd);
int grid_idsva_so_host(grid_handle *h, const float *h_q_qd_u, const float *h_qdd, int num_timesteps, float gravity, float *h_idsva_so);
int grid_fdsva_so_host(grid_handle *h, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_df2);
int grid_forward_dynamics_gradient_qdd_minv_host(grid_handle *h, const float *h_q_qd, int stride_q_qd, const float *h_qdd, const float *h_Minv, int num_timesteps,
                                                 float gravity, float *h_df_du);

/* Multi-GPU form of the hot path: ONE host batch of num_timesteps solves is cut into num_handles
 * contiguous ranges of ceil(num_timesteps/num_handles) solves, range g runs on handles[g] (one handle per GPU, one host thread per handle:
 * H2D, kernel, D2H on that handle's stream), results land in the matching ranges of h_df_du.  No collective: every solve is independent
 * (reference helpers/_code_generation_helpers.py:46-47, the kernels' only cross-k structure is the grid-stride loop).  Synchronous. */
int grid_forward_dynamics_gradient_multi_host(grid_handle **handles, int num_handles, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_df_du);

/* T = double instantiations (reference: template <typename T> on every emitted function, GRiDCodeGenerator.py:312-380): the same entry points with
 * double buffers and a double gravity; their device and pinned host buffers are allocated by the first *_f64 call on a handle.  A block never asks
 * for more LDS than a CU has: where the float block size does not fit in double precision the library launches fewer solves per block. */
int grid_forward_dynamics_gradient_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, int num_timesteps, double gravity,
                                              double *d_df_du, void *stream);
int grid_forward_dynamics_gradient_qdd_minv_device_f64(grid_handle *h, const double *d_q_qd, int stride_q_qd, const double *d_qdd, const double *d_Minv,
                                                       int num_timesteps, double gravity, double *d_df_du, void *stream);
int grid_inverse_dynamics_device_f64(grid_handle *h, const double *d_q_qd, int stride_q_qd, const double *d_qdd, int num_timesteps, double gravity,
                                     double *d_c, void *stream);
int grid_inverse_dynamics_gradient_device_f64(grid_handle *h, const double *d_q_qd, int stride_q_qd, const double *d_qdd, int num_timesteps, double gravity,
                                              double *d_dc_du, void *stream);
int grid_direct_minv_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_Minv, void *stream);
int grid_forward_dynamics_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, int num_timesteps, double gravity, double *d_qdd, void *stream);
int grid_aba_device_f64(grid_handle *h, const double *d_q_qd_tau, int stride_q_qd, int num_timesteps, double gravity, double *d_qdd, void *stream);
int grid_idsva_so_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, const double *d_qdd, int num_timesteps, double gravity,
                             double *d_idsva_so, void *stream);
int grid_fdsva_so_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, int num_timesteps, double gravity, double *d_df2, void *stream);
int grid_forward_dynamics_gradient_host_f64(grid_handle *h, const double *h_q_qd_u, int num_timesteps, double gravity, double *h_df_du);
int grid_inverse_dynamics_host_f64(grid_handle *h, const double *h_q_qd, int stride_q_qd, const double *h_qdd, int num_timesteps, double gravity, double *h_c);
int grid_inverse_dynamics_gradient_host_f64(grid_handle *h, const double *h_q_qd, int stride_q_qd, const double *h_qdd, int num_timesteps, double gravity, double *h_dc_du);
int grid_direct_minv_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_Minv);
int grid_forward_dynamics_host_f64(grid_handle *h, const double *h_q_qd_u, int num_timesteps, double gravity, double *h_qdd);
int grid_aba_host_f64(grid_handle *h, const double *h_q_qd_tau, int num_timesteps, double gravity, double *h_qdd);
int grid_idsva_so_host_f64(grid_handle *h, const double *h_q_qd_u, const double *h_qdd, int num_timesteps, double gravity, double *h_idsva_so);
int grid_fdsva_so_host_f64(grid_handle *h, const double *h_q_qd_u, int num_timesteps, double gravity, double *h_df2);

/* End-effector kinematics (reference algorithms/_eepose_gradient_hessian.py, emitted by the reference's gen_all_code for every fixed-base robot).
 * Every leaf joint is an end effector (ascending id); the pose of one is [x, y, z, roll, pitch, yaw] of its link frame in the base frame (no tool offset).
 * Layouts (k = batch index):  eePos [k*6E + 6e + c],  deePos [k*6En + 6(e*n + j) + c],  d2eePos [k*6En^2 + e*6n^2 + c*n^2 + i*n + j]
 * (the reference's Hessian layout for E = 1; for E > 1 every end effector has its own 6n^2 block - the reference's offsets overlap them).
 * q is read with a caller stride >= n (n: the reference's USE_COMPRESSED_MEM, 3n: q_qd_u).  No gravity argument (kinematics). */
int grid_num_end_effectors(void);
int grid_end_effector_joints(int *out); /* writes the grid_num_end_effectors() leaf joint ids */
/* replace end_effector_pose_kernel<T> / end_effector_pose_gradient_kernel<T> / end_effector_pose_gradient_hessian_kernel<T>
 * (reference algorithms/_eepose_gradient_hessian.py: gen_end_effector_pose_kernel, _gradient_kernel, _gradient_hessian_kernel): device buffers, asynchronous
 * on `stream`, nothing allocated.  d_deePos of the Hessian entry point may be NULL (otherwise it receives the gradient, as the reference's kernel writes both) */
int grid_end_effector_pose_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_eePos, void *stream);
int grid_end_effector_pose_gradient_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_deePos, void *stream);
int grid_end_effector_pose_gradient_hessian_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_d2eePos, float *d_deePos, void *stream);
/* replace the host wrappers end_effector_pose<T,USE_COMPRESSED_MEM> / end_effector_pose_gradient<T,...> / end_effector_pose_gradient_hessian<T,...>
 * (reference algorithms/_eepose_gradient_hessian.py: gen_end_effector_pose_host and its twins): host buffers, synchronous, num_timesteps <= max_timesteps.
 * Their device staging is allocated by the first kinematics call on a handle; the Hessian's is at most 1 GiB and longer batches pass through it in chunks.
 * h_deePos of the Hessian entry point may be NULL. */
int grid_end_effector_pose_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_eePos);
int grid_end_effector_pose_gradient_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_deePos);
int grid_end_effector_pose_gradient_hessian_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_d2eePos, float *h_deePos);
int grid_end_effector_pose_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_eePos, void *stream);
int grid_end_effector_pose_gradient_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_deePos, void *stream);
int grid_end_effector_pose_gradient_hessian_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_d2eePos, double *d_deePos, void *stream);
int grid_end_effector_pose_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_eePos);
int grid_end_effector_pose_gradient_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_deePos);
int grid_end_effector_pose_gradient_hessian_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_d2eePos, double *h_deePos);

/* Joint-space inertia matrix M(q) (reference algorithms/_crba.py, emitted by the reference's gen_all_code for every fixed-base robot).
 * Layout (k = batch index): M[k*n*n + col*n + row], dense (both triangles, structural zeros included); exactly symmetric.
 * q is the first n values of every row (stride n, 2n: the reference's USE_COMPRESSED_MEM q_qd, 3n: q_qd_u).  No gravity argument: M does not depend on it. */
/* replaces crba_kernel<T> (reference algorithms/_crba.py: gen_crba_kernel): device buffers, asynchronous on `stream`, nothing allocated; stride_q >= n */
int grid_crba_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_M, void *stream);
/* replaces the host wrapper crba<T,USE_COMPRESSED_MEM> (reference algorithms/_crba.py: gen_crba_host): host buffers, synchronous, stride_q in [n, 3n],
 * num_timesteps <= max_timesteps.  The output is staged in the handle's own d_M buffer, allocated by the first call. */
int grid_crba_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_M);
int grid_crba_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_M, void *stream);
int grid_crba_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_M);

/* Fused rollout: num_steps steps of ABA forward dynamics + semi-implicit (symplectic) Euler for num_solves independent trajectories in ONE launch, the
 * state resident in LDS between the steps.  The reference has no counterpart (its user launches aba_kernel once per step and integrates in between).
 *   qdd = ABA(q_t, qd_t, u_t);  qd_{t+1} = qd_t + dt*qdd;  q_{t+1} = q_t + dt*qd_{t+1}   (no joint limits, no angle wrapping, no contact)
 * Layouts (n joints, k = solve, t = step; time-major):
 *   x0    rows of stride_x0 >= 2n values whose first 2n are [q | qd] (the 3n q_qd_u rows of the other entry points are accepted as they are)
 *   u     element (t, k, j) at u[t*stride_u_step + k*stride_u_solve + j]; dense (num_steps, num_solves, n): stride_u_solve = n, stride_u_step = num_solves*n;
 *         stride_u_solve = 0: ONE sequence (num_steps, n) for all solves.  Otherwise stride_u_solve >= n, and stride_u_step covers what one step spans
 *   traj  (num_steps+1, num_solves, 2n), traj[t][k] = [q_t | qd_t], row 0 is x0; may be NULL: nothing is written during the steps
 *   xT    (num_solves, 2n), the final state; may be NULL.  At least one of traj and xT must be given.
 * num_steps == 0 copies x0 to the outputs.  Negative counts, NULL inputs, both outputs NULL and bad strides are errors (grid_last_error). */
/* no counterpart in the reference (launches rollout_kernel<T>): device buffers, asynchronous on `stream`, nothing allocated */
int grid_rollout_device(grid_handle *h, const float *d_x0, int stride_x0, const float *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                        float dt, float gravity, float *d_traj, float *d_xT, void *stream);
/* no counterpart in the reference: host buffers, synchronous, stride_x0 in [2n, 3n], num_solves <= max_timesteps.  u and traj / xT are staged in device
 * buffers of the handle that the first call allocates and longer calls grow; grid_close frees them. */
int grid_rollout_host(grid_handle *h, const float *h_x0, int stride_x0, const float *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                      float dt, float gravity, float *h_traj, float *h_xT);
int grid_rollout_device_f64(grid_handle *h, const double *d_x0, int stride_x0, const double *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                            double dt, double gravity, double *d_traj, double *d_xT, void *stream);
int grid_rollout_host_f64(grid_handle *h, const double *h_x0, int stride_x0, const double *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                          double dt, double gravity, double *h_traj, double *h_xT);

/* Linearised rollout: the fused rollout AND the Jacobians of the dynamics along it, ONE launch, one dynamics pass per step (the factorisation of M inside the
 * forward-dynamics-gradient pass gives qdd; its trajectory agrees with grid_rollout_*'s, which runs ABA, to rounding - not bit for bit).  Per solve and step:
 *   qdd_t = FD(q_t, qd_t, u_t);  fx_t = [d qdd/dq | d qdd/dqd];  fu_t = d qdd/du = M^-1(q_t);  then the semi-implicit Euler update of grid_rollout_*
 * x0, u, traj, xT and their strides exactly as grid_rollout_*, followed by
 *   fx    (num_steps, num_solves, 2n^2): the df_du record of grid_forward_dynamics_gradient_* at (x_t, u_t), fx[col*n + row]; may be NULL
 *   fu    (num_steps, num_solves, n^2): dense, exactly symmetric, fu[col*n + row]; may be NULL (the work that only M^-1 needs is then skipped)
 * At least one of the four outputs must be given.  The discrete Jacobians of the step map x = [q; qd] follow without further dynamics (Fq | Fv = fx):
 *   A_t = [[I + dt^2 Fq, dt (I + dt Fv)], [dt Fq, I + dt Fv]],  B_t = [[dt^2 fu], [dt fu]]
 * num_steps == 0 copies x0 to traj / xT and writes no Jacobian.  Errors as grid_rollout_*. */
/* no counterpart in the reference (launches rollout_linearized_kernel<T>): device buffers, asynchronous on `stream`, nothing allocated */
int grid_rollout_linearized_device(grid_handle *h, const float *d_x0, int stride_x0, const float *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                                   float dt, float gravity, float *d_traj, float *d_xT, float *d_fx, float *d_fu, void *stream);
/* no counterpart in the reference: host buffers, synchronous, stride_x0 in [2n, 3n], num_solves <= max_timesteps.  Everything is staged in device buffers of the
 * handle that the first call allocates and longer calls grow; grid_close frees them.  Each staged output is capped at GRID_ROLLOUT_LIN_HOST_CAP_BYTES (1 GiB):
 * a call whose fx (or fu, traj) record would be larger returns hipErrorInvalidValue with a grid_last_error text and leaves the handle usable - split the
 * horizon (the final state of one call is the x0 of the next) or use the device entry point with buffers of your own. */
#define GRID_ROLLOUT_LIN_HOST_CAP_BYTES ((size_t)1 << 30)
int grid_rollout_linearized_host(grid_handle *h, const float *h_x0, int stride_x0, const float *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                                 float dt, float gravity, float *h_traj, float *h_xT, float *h_fx, float *h_fu);
int grid_rollout_linearized_device_f64(grid_handle *h, const double *d_x0, int stride_x0, const double *d_u, long stride_u_step, int stride_u_solve, int num_solves,
                                       int num_steps, double dt, double gravity, double *d_traj, double *d_xT, double *d_fx, double *d_fu, void *stream);
int grid_rollout_linearized_host_f64(grid_handle *h, const double *h_x0, int stride_x0, const double *h_u, long stride_u_step, int stride_u_solve, int num_solves,
                                     int num_steps, double dt, double gravity, double *h_traj, double *h_xT, double *h_fx, double *h_fu);

/* Rollout adjoint: the gradient of a scalar cost of a trajectory, L = sum_t l_t(x_t), with respect to x0 and every u_t, ONE launch in reverse time.  The caller has
 * rolled out (grid_rollout_* or grid_rollout_linearized_*) and hands back what that call read and wrote, together with g_t = d l_t / d x_t.  Per solve, with the discrete
 * Jacobians A_t, B_t of grid_rollout_linearized_*:
 *   lam_T = g_T;   t = T-1 .. 0:  grad_u_t = B_t^T lam_{t+1},  lam_t = g_t + A_t^T lam_{t+1};   grad_x0 = lam_0
 * Every step is re-linearised on chip at (traj[t], u[t]) and contracted with lam on the spot: no n^2-sized record is written.  Cost terms in u are the caller's own.
 *   traj    (num_steps+1, num_solves, 2n): the states the rollout wrote for u (row num_steps is not read; with num_steps == 0 neither traj nor u is)
 *   u       element (t, k, j) at u[t*stride_u_step + k*stride_u_solve + j]; strides as grid_rollout_*; stride_u_solve == 0: one sequence for all solves
 *   gx      (num_steps+1, num_solves, 2n): d cost / d traj; may be NULL
 *   gxT     (num_solves, 2n): d cost / d x_T; may be NULL; at least one of gx, gxT; where both are given gxT is added to row num_steps of gx
 *   grad_x0 (num_solves, 2n); may be NULL
 *   grad_u  (num_steps, num_solves, n): always per solve - for a shared control sequence the caller sums over the solves; may be NULL (the work only M^-1 needs
 *           is then skipped); at least one of grad_x0, grad_u
 * num_steps == 0 gives grad_x0 = gx[0] (+ gxT) and writes no grad_u.  Errors (return code != 0, text in grid_last_error, handle stays usable): negative counts, NULL traj or
 * u with num_steps > 0, both cotangents NULL, both outputs NULL, a solve stride that is neither 0 nor >= n, a step stride shorter than one step spans. */
/* no counterpart in the reference (launches rollout_adjoint_kernel<T>): device buffers, asynchronous on `stream`, nothing allocated */
int grid_rollout_adjoint_device(grid_handle *h, const float *d_traj, const float *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, float dt, float gravity,
                                const float *d_gx, const float *d_gxT, float *d_grad_x0, float *d_grad_u, void *stream);
/* no counterpart in the reference: host buffers, synchronous, num_solves <= max_timesteps.  Everything is staged in device buffers of the handle that the first call
 * allocates and longer calls grow; grid_close frees them.  Each staged record is capped at GRID_ROLLOUT_LIN_HOST_CAP_BYTES (1 GiB): a longer call returns
 * hipErrorInvalidValue with a grid_last_error text before anything is allocated and leaves the handle usable - use the device entry point with buffers of your own. */
int grid_rollout_adjoint_host(grid_handle *h, const float *h_traj, const float *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, float dt, float gravity,
                              const float *h_gx, const float *h_gxT, float *h_grad_x0, float *h_grad_u);
int grid_rollout_adjoint_device_f64(grid_handle *h, const double *d_traj, const double *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, double dt,
                                    double gravity, const double *d_gx, const double *d_gxT, double *d_grad_x0, double *d_grad_u, void *stream);
int grid_rollout_adjoint_host_f64(grid_handle *h, const double *h_traj, const double *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, double dt,
                                  double gravity, const double *h_gx, const double *h_gxT, double *h_grad_x0, double *h_grad_u);

/* Closed-loop rollout: the fused rollout with the control of every step formed INSIDE the step loop from the state the rollout has just reached - a time-varying
 * linear feedback law and, optionally, torque limits.  Per solve k and step t (dynamics, gravity convention, damping and integrator of grid_rollout_*):
 *   dx  = x_t - x_ref[t, k]                               x = [q ; qd], 2n values
 *   v   = u_ff[t, k][j] + sum_c K[t, k][c*n + j]*dx[c]    one accumulator per joint j that starts from u_ff, c ascending 0 .. 2n-1
 *   u_t = v, or with limits  v < u_min[j] ? u_min[j] : (v > u_max[j] ? u_max[j] : v)      (a NaN v stays NaN)
 *   qdd = ABA(q_t, qd_t, u_t), then the semi-implicit Euler update of grid_rollout_*
 * (iLQR / DDP forward pass: u_ff = u_bar + alpha*k, x_ref = the nominal trajectory.)  Layouts, time-major:
 *   x0, traj, xT   exactly as grid_rollout_*
 *   u_ff    as the u of grid_rollout_*: element (t, k, j) at u_ff[t*stride_u_step + k*stride_u_solve + j], same stride rules (stride_u_solve == 0: shared)
 *   K       element (t, k, c*n + j) at K[t*stride_K_step + k*stride_K_solve + c*n + j]: the n x 2n gain stored [col*n + row] like every matrix of the library.
 *           stride_K_step == 0: one gain for all steps; stride_K_solve == 0: one gain for all solves; otherwise stride_K_solve >= 2n^2 and stride_K_step
 *           covers what one step spans.  Dense (num_steps, num_solves, 2n^2): stride_K_solve = 2n^2, stride_K_step = num_solves*2n^2
 *   x_ref   element (t, k, i), i < 2n, at x_ref[t*stride_xref_step + k*stride_xref_solve + i].  stride_xref_step == 0: set-point regulation; stride_xref_solve == 0:
 *           one reference for all solves; otherwise stride_xref_solve >= 2n and stride_xref_step covers what one step spans.  A nominal traj (num_steps+1,
 *           num_solves, 2n) of grid_rollout_* passes as it is (row num_steps is not read)
 *   u_min, u_max   n values each, shared by all solves and steps; both given or both NULL (no limits)
 *   u_out   (num_steps, num_solves, n): the control that was applied, after the limits; may be NULL
 * Every output may be NULL, but not all three.  num_steps == 0 copies x0 to traj / xT, writes no u_out and reads neither K nor x_ref.
 * Errors (return code != 0, text in grid_last_error, handle stays usable): everything grid_rollout_* refuses, NULL K or x_ref with num_steps > 0, exactly one of
 * u_min / u_max, all three outputs NULL, a K or x_ref solve stride that is neither 0 nor at least one record, a step stride that is neither 0 nor at least what one
 * step spans, negative strides. */
/* no counterpart in the reference (launches rollout_feedback_kernel<T>): device buffers, asynchronous on `stream`, nothing allocated */
int grid_rollout_feedback_device(grid_handle *h, const float *d_x0, int stride_x0, const float *d_u_ff, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                                 float dt, float gravity, const float *d_K, long stride_K_step, long stride_K_solve, const float *d_x_ref, long stride_xref_step,
                                 long stride_xref_solve, const float *d_u_min, const float *d_u_max, float *d_traj, float *d_xT, float *d_u_out, void *stream);
/* no counterpart in the reference: host buffers, synchronous, stride_x0 in [2n, 3n], num_solves <= max_timesteps.  Everything is staged in device buffers of the
 * handle that the first call allocates and longer calls grow (a shared or time-invariant K / x_ref is staged once); grid_close frees them.  Each staged record is
 * capped at GRID_ROLLOUT_LIN_HOST_CAP_BYTES (1 GiB): a longer call returns hipErrorInvalidValue with a grid_last_error text before anything is allocated. */
int grid_rollout_feedback_host(grid_handle *h, const float *h_x0, int stride_x0, const float *h_u_ff, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                               float dt, float gravity, const float *h_K, long stride_K_step, long stride_K_solve, const float *h_x_ref, long stride_xref_step,
                               long stride_xref_solve, const float *h_u_min, const float *h_u_max, float *h_traj, float *h_xT, float *h_u_out);
int grid_rollout_feedback_device_f64(grid_handle *h, const double *d_x0, int stride_x0, const double *d_u_ff, long stride_u_step, int stride_u_solve, int num_solves,
                                     int num_steps, double dt, double gravity, const double *d_K, long stride_K_step, long stride_K_solve, const double *d_x_ref,
                                     long stride_xref_step, long stride_xref_solve, const double *d_u_min, const double *d_u_max, double *d_traj, double *d_xT,
                                     double *d_u_out, void *stream);
int grid_rollout_feedback_host_f64(grid_handle *h, const double *h_x0, int stride_x0, const double *h_u_ff, long stride_u_step, int stride_u_solve, int num_solves,
                                   int num_steps, double dt, double gravity, const double *h_K, long stride_K_step, long stride_K_solve, const double *h_x_ref,
                                   long stride_xref_step, long stride_xref_solve, const double *h_u_min, const double *h_u_max, double *h_traj, double *h_xT,
                                   double *h_u_out);

/* in-kernel timing probe: replaces forward_dynamics_gradient_single_timing<T> (reference :236-248); returns microseconds per solve */
int grid_forward_dynamics_gradient_single_timing(grid_handle *h, const float *h_q_qd_u, int reps, float gravity, float *h_df_du, double *us_per_call);

#ifdef __cplusplus
}
#endif
#endif /* GRID_CAPI_H */
