// grid_capi.hip - C-ABI shim over the generated, robot-specialised HIP header (see include/grid_capi.h).
// Built once per robot:  hipcc --offload-arch=gfx950 -O3 -shared -fPIC -I<dir of generated grid.cuh> -I<repo>/include grid_capi.hip
//
// Error model: the generated host API follows the reference (gpuAssert prints and exit()s, reference GRiDCodeGenerator.py:279-286).
// This library must never take the host process down, so it re-binds the header's error hook to a C++ exception that every
// entry point catches and turns into the hipError_t return value.
#include <hip/hip_runtime.h>

struct grid_capi_error {
    hipError_t code;
    const char *file;
    int line;
};
#define GRID_ON_GPU_ERROR(code, file, line) throw grid_capi_error{(code), (file), (line)}

#include "grid.cuh"
#include "grid_capi.h"

#include <limits.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#ifndef GRID_ROBOT_NAME
#define GRID_ROBOT_NAME "robot"
#endif

template <typename T>
struct grid_typed {
    grid::robotModel<T> *d_robotModel = nullptr;
    grid::gridData<T> *hd_data = nullptr;
    size_t M_cap = 0;  // elements of hd_data->d_M, the output staging of the crba host entry point (allocated by its first call; no pinned twin)
    size_t u_traj_cap = 0, x_traj_cap = 0;  // elements of hd_data->d_u_traj / d_x_traj, the staging of the rollout host entry point (same rules)
    size_t fx_traj_cap = 0, fu_traj_cap = 0;  // elements of hd_data->d_fx_traj / d_fu_traj, the Jacobian staging of the linearised rollout host entry point (same rules)
    size_t gx_traj_cap = 0, gu_traj_cap = 0, gx0_cap = 0;  // elements of hd_data->d_gx_traj / d_gu_traj / d_gx0, the staging of the rollout adjoint host entry point (same rules)
    size_t K_traj_cap = 0, xref_traj_cap = 0, uout_traj_cap = 0, u_lim_cap = 0;  // elements of hd_data->d_K_traj / d_xref_traj / d_uout_traj / d_u_lim, the staging of the closed-loop rollout host entry point (same rules)
};

// staging of the kinematics host entry points (grid_end_effector_pose*_host): allocated by the first kinematics call on a handle, never by grid_init,
// and grown when a later call needs more; capacities in elements of T
template <typename T>
struct ee_stage {
    T *d_q = nullptr, *d_out = nullptr, *d_dee = nullptr;
    size_t q_cap = 0, out_cap = 0, dee_cap = 0;
};

struct grid_handle {
    int device;
    int max_timesteps;
    int blocks;   // 0 = derive from the batch
    int threads;  // 0 = the kernel's suggested block size
    int host_chunks;  // 0 = automatic: chunks of the pipelined host entry point (page-locked buffers)
    hipStream_t *streams;
    grid_typed<float> f32;
    grid_typed<double> f64;  // allocated by the first *_f64 call
    std::mutex alloc_lock;   // serialises that lazy allocation (two threads making their first *_f64 call on one handle)
    // GRID_SO_DIRECT (records beyond the LDS of a CU): fdsva_so keeps the idsva_so tensors in the handle's ONE d_idsva_so workspace.  Calls on different streams
    // (or threads) are made safe by ordering them: every launch waits for the previous one's event before it may touch the workspace
    hipEvent_t so_done = nullptr;
    bool so_pending = false;
    ee_stage<float> ee32;
    ee_stage<double> ee64;
};
template <typename T> static inline grid_typed<T> &typed(grid_handle *h);
template <> inline grid_typed<float> &typed<float>(grid_handle *h) { return h->f32; }
template <> inline grid_typed<double> &typed<double>(grid_handle *h) { return h->f64; }

template <typename T> static inline ee_stage<T> &ee_staging(grid_handle *h);
template <> inline ee_stage<float> &ee_staging<float>(grid_handle *h) { return h->ee32; }
template <> inline ee_stage<double> &ee_staging<double>(grid_handle *h) { return h->ee64; }

static thread_local char g_err[512] = "";

static int fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}
static int fail_msg(hipError_t e, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return (int)e;
}
#define GRID_TRY(expr)                                   \
    do {                                                 \
        hipError_t e__ = (expr);                         \
        if (e__ != hipSuccess) return fail(e__, #expr);  \
    } while (0)
// every entry point body runs inside this: errors raised by the generated host API come back as return codes
#define GRID_GUARDED(body)                                                                                                       \
    try {                                                                                                                        \
        body                                                                                                                     \
    } catch (const grid_capi_error &e) {                                                                                         \
        snprintf(g_err, sizeof(g_err), "%s (%s:%d)", hipGetErrorString(e.code), e.file, e.line);                                 \
        return (int)e.code;                                                                                                      \
    } catch (const std::exception &e) {                                                                                          \
        snprintf(g_err, sizeof(g_err), "%s", e.what());                                                                          \
        return (int)hipErrorUnknown;                                                                                             \
    }

// Makes the handle's device current for the duration of a call and restores the caller's device afterwards: one process may hold
// one handle per GPU and call them from any thread in any order (reference: one implicit device, default-stream launches).
struct device_guard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit device_guard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = (err == hipSuccess);
        }
    }
    ~device_guard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define GRID_ON_DEVICE(h)                  \
    device_guard guard__((h)->device);     \
    if (guard__.err != hipSuccess) return fail(guard__.err, "hipSetDevice(handle device)")

static const size_t GRID_CU_LDS_BYTES = 160 * 1024;  // LDS of one gfx950 CU: no block may ask for more

// launch geometry of one kernel: lane groups per block (capped by the kernel's own limit and by the CU's LDS), threads, blocks, LDS bytes
struct launch_cfg {
    dim3 grid, block;
    size_t lds;
};
// the second-order kernels: robots with 8-lane groups carry a second instance of the library for 16-lane groups (GRID_SO_WIDE, namespace grid::wide)
#ifdef GRID_SO_WIDE
namespace grid_so = grid::wide;
#else
namespace grid_so = grid;
#endif

// what the launch geometry of one kernel is derived from: the constants the generated header emits beside it.  threads: its suggested block size; max_groups: the
// lane groups per block it serves (it retires the rest); lds, out: elements of one solve's LDS slice and of its output staging; lanes: lanes of one lane group
struct kernel_shape {
    int threads, max_groups, lds, out, lanes;
};
namespace shape {
constexpr kernel_shape outer(int threads, int lds, int out) { return {threads, grid::GRID_MAX_SOLVES_PER_BLOCK, lds, out, grid::GRID_LANES_PER_SOLVE}; }
constexpr kernel_shape GENERAL = outer(grid::SUGGESTED_THREADS, grid::GRID_LDS_PER_SOLVE, grid::GRID_OUT_PER_SOLVE);  // the kernels without a slice of their own
// forward_dynamics_gradient_kernel has its own (smaller) LDS slice and suggested block size
constexpr kernel_shape FD_DU = outer(grid::FD_DU_SUGGESTED_THREADS, grid::FD_DU_LDS_PER_SOLVE, grid::FD_DU_OUT_PER_SOLVE);
constexpr kernel_shape ID = outer(grid::ID_SUGGESTED_THREADS, grid::ID_LDS_PER_SOLVE, grid::ID_OUT_PER_SOLVE);
constexpr kernel_shape ID_DU = outer(grid::ID_DU_SUGGESTED_THREADS, grid::ID_DU_LDS_PER_SOLVE, grid::ID_DU_OUT_PER_SOLVE);
constexpr kernel_shape MINV = outer(grid::MINV_SUGGESTED_THREADS, grid::MINV_LDS_PER_SOLVE, grid::MINV_OUT_PER_SOLVE);
constexpr kernel_shape FD = outer(grid::FD_SUGGESTED_THREADS, grid::FD_LDS_PER_SOLVE, grid::FD_OUT_PER_SOLVE);
constexpr kernel_shape ABA = outer(grid::ABA_SUGGESTED_THREADS, grid::ABA_LDS_PER_SOLVE, grid::ABA_OUT_PER_SOLVE);
constexpr kernel_shape CRBA = outer(grid::CRBA_SUGGESTED_THREADS, grid::CRBA_LDS_PER_SOLVE, grid::CRBA_OUT_PER_SOLVE);
// end-effector kinematics: pose, gradient, Hessian (the `which` of ee_device)
constexpr kernel_shape EE[3] = {outer(grid::EE_POS_SUGGESTED_THREADS, grid::EE_POS_LDS_PER_SOLVE, grid::EE_POS_OUT_PER_SOLVE),
                                outer(grid::DEE_POS_SUGGESTED_THREADS, grid::DEE_POS_LDS_PER_SOLVE, grid::DEE_POS_OUT_PER_SOLVE),
                                outer(grid::D2EE_POS_SUGGESTED_THREADS, grid::D2EE_POS_LDS_PER_SOLVE, grid::D2EE_POS_OUT_PER_SOLVE)};
constexpr kernel_shape ROLLOUT = outer(grid::ROLLOUT_SUGGESTED_THREADS, grid::ROLLOUT_LDS_PER_SOLVE, grid::ROLLOUT_OUT_PER_SOLVE);
constexpr kernel_shape ROLLOUT_LIN = outer(grid::ROLLOUT_LIN_SUGGESTED_THREADS, grid::ROLLOUT_LIN_LDS_PER_SOLVE, grid::ROLLOUT_LIN_OUT_PER_SOLVE);
constexpr kernel_shape ROLLOUT_ADJ = outer(grid::ROLLOUT_ADJ_SUGGESTED_THREADS, grid::ROLLOUT_ADJ_LDS_PER_SOLVE, grid::ROLLOUT_ADJ_OUT_PER_SOLVE);
constexpr kernel_shape ROLLOUT_FB = outer(grid::ROLLOUT_FB_SUGGESTED_THREADS, grid::ROLLOUT_FB_LDS_PER_SOLVE, grid::ROLLOUT_FB_OUT_PER_SOLVE);
#if GRID_HAS_IDSVA_SO
// (the second-order kernels of 8-lane robots run 16-lane groups: namespace wide)
constexpr kernel_shape IDSVA_SO{grid_so::IDSVA_SO_SUGGESTED_THREADS, grid_so::IDSVA_SO_MAX_SOLVES_PER_BLOCK, grid_so::IDSVA_SO_LDS_PER_SOLVE, grid_so::IDSVA_SO_STAGE_PER_SOLVE, grid_so::GRID_LANES_PER_SOLVE};
constexpr kernel_shape FDSVA_SO{grid_so::FDSVA_SO_SUGGESTED_THREADS, grid_so::FDSVA_SO_MAX_SOLVES_PER_BLOCK, grid_so::FDSVA_SO_LDS_PER_SOLVE, grid_so::FDSVA_SO_STAGE_PER_SOLVE, grid_so::GRID_LANES_PER_SOLVE};
#endif
}  // namespace shape

template <typename T>
static int make_launch(const grid_handle *h, int num_timesteps, const kernel_shape &k, launch_cfg *cfg) {
    int threads = h->threads > 0 ? h->threads : k.threads;
    if (threads < k.lanes) threads = k.lanes;  // (the second-order kernels of 8-lane robots run 16-lane groups: namespace wide)
    if (threads < grid::GRID_MIN_THREADS || threads > grid::GRID_MAX_THREADS)
        return fail_msg(hipErrorInvalidConfiguration, "threads per block out of range");
    if (k.lanes == grid::GRID_LANES_PER_SOLVE) threads -= threads % grid::GRID_MIN_THREADS;  // (GRID_LANE_INTERLEAVE: blocks are whole 16-lane rows; the kernels retire the rest)
    int gpb = threads / k.lanes;
    if (gpb > k.max_groups) gpb = k.max_groups;  // (the kernels retire the lane groups beyond their cap)
    const size_t per_group = (size_t)(k.lds + k.out) * sizeof(T);
    if ((size_t)gpb * per_group > GRID_CU_LDS_BYTES) {
        // e.g. the 30-DoF robot in double precision: fewer solves per block than the block size suggests
        gpb = (int)(GRID_CU_LDS_BYTES / per_group);
        if (gpb < 1) return fail_msg(hipErrorInvalidConfiguration, "one solve of this robot does not fit the LDS of a CU in this precision");
        threads = gpb * k.lanes;
    }
    int blocks = h->blocks > 0 ? h->blocks : (num_timesteps + gpb - 1) / gpb;
    if (blocks < 1) blocks = 1;
    cfg->grid = dim3(blocks, 1, 1);
    cfg->block = dim3(threads, 1, 1);
    cfg->lds = (size_t)gpb * per_group;
    return 0;
}

static int check_args(const grid_handle *h, int num_timesteps) {
    if (!h) return fail_msg(hipErrorInvalidValue, "null handle");
    if (num_timesteps < 0) return fail_msg(hipErrorInvalidValue, "negative num_timesteps");
    if (h->threads != 0 && (h->threads < grid::GRID_MIN_THREADS || h->threads > grid::GRID_MAX_THREADS)) {
        snprintf(g_err, sizeof(g_err), "threads per block must be in [%d, %d]", grid::GRID_MIN_THREADS, grid::GRID_MAX_THREADS);
        return (int)hipErrorInvalidConfiguration;
    }
    return 0;
}

// device entry points with one strided input and one output: check_args, then: required pointers must not be NULL and the stride must cover what the kernel loads per
// solve (a smaller or negative stride would make the last solves read before / past the caller's buffer: a GPU memory fault instead of an error code)
static int check_device_io(const grid_handle *h, const void *in, int stride, int min_stride, const void *out, int num_timesteps) {
    const int rc = check_args(h, num_timesteps);
    if (rc || num_timesteps == 0) return rc;
    if (!in || !out) return fail_msg(hipErrorInvalidValue, "null input or output pointer");
    if (stride < min_stride) {
        snprintf(g_err, sizeof(g_err), "stride %d is smaller than the %d values the kernel reads per solve", stride, min_stride);
        return (int)hipErrorInvalidValue;
    }
    return 0;
}

// device + pinned host bytes init_gridData<T>(N) will ask for (same list as the generated function)
template <typename T>
static size_t grid_data_bytes(int N) {
    const size_t n = grid::NUM_JOINTS;
    size_t per = 3 * n + 2 * n + n + n + n * n + n + 2 * n * n + 2 * n * n;
    size_t bytes = per * (size_t)N * sizeof(T);
#if GRID_HAS_IDSVA_SO
    const int so = N < grid::grid_so_max_timesteps<T>() ? N : grid::grid_so_max_timesteps<T>();
    bytes += 8 * n * n * n * (size_t)so * sizeof(T);
#endif
    return bytes;
}

// solves per call the second-order entry points of this handle accept (their records are 4 n^3 values: init_gridData caps those buffers)
template <typename T>
static int so_capacity(const grid_handle *h) {
#if GRID_HAS_IDSVA_SO
    return h->max_timesteps < grid::grid_so_max_timesteps<T>() ? h->max_timesteps : grid::grid_so_max_timesteps<T>();
#else
    (void)h;
    return 0;
#endif
}

template <typename T>
static int ensure_typed(grid_handle *h) {
    grid_typed<T> &t = typed<T>(h);
    std::lock_guard<std::mutex> lock(h->alloc_lock);
    if (t.hd_data) return 0;
    size_t free_b = 0, total_b = 0;
    GRID_TRY(hipMemGetInfo(&free_b, &total_b));
    if (grid_data_bytes<T>(h->max_timesteps) > free_b) {
        snprintf(g_err, sizeof(g_err), "grid_init: max_timesteps = %d needs %zu bytes of device memory, %zu are free", h->max_timesteps,
                 grid_data_bytes<T>(h->max_timesteps), free_b);
        return (int)hipErrorOutOfMemory;
    }
    if (!t.d_robotModel) t.d_robotModel = grid::init_robotModel<T>();
    t.hd_data = grid::init_gridData<T>(h->max_timesteps);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- device entry points
// What every device entry point does between the checks of its own arguments (`checked`: what they returned) and its launch.  A failed check or N == 0 ends the
// call with rc, before the device is switched and before anything is allocated.  Otherwise the handle's device is made current (and the caller's restored when
// this object goes: it lives across the launch), the handle's state for T is allocated on first use and the launch geometry of the kernel is worked out.
// ready: the caller launches; else it returns rc (grid_last_error is set where rc != 0).
template <typename T>
struct device_launch : launch_cfg {
    std::optional<device_guard> guard;
    const grid::robotModel<T> *model = nullptr;
    int rc;
    bool ready = false;
    device_launch(grid_handle *h, int N, const kernel_shape &k, int checked) : rc(checked) {
        if (rc || N == 0) return;
        guard.emplace(h->device);
        rc = guard->err != hipSuccess ? fail(guard->err, "hipSetDevice(handle device)") : ensure_typed<T>(h);
        if (!rc) rc = make_launch<T>(h, N, k, this);
        if (!rc) model = typed<T>(h).d_robotModel;
        ready = !rc;
    }
};
// ... and after it
static int launch_status() {
    GRID_TRY(hipGetLastError());
    return 0;
}

template <typename T>
static int fd_grad_device(grid_handle *h, const T *d_q_qd_u, int stride, int N, T gravity, T *d_df_du, void *stream) {
    device_launch<T> L(h, N, shape::FD_DU, check_device_io(h, d_q_qd_u, stride, 3*(int)grid::NUM_JOINTS, d_df_du, N));
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::forward_dynamics_gradient_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_df_du, d_q_qd_u, stride, L.model, gravity, N);
    return launch_status();
}

template <typename T>
static int fd_grad_qdd_minv_device(grid_handle *h, const T *d_q_qd, int stride, const T *d_qdd, const T *d_Minv, int N, T gravity, T *d_df_du, void *stream) {
    int rc = check_device_io(h, d_q_qd, stride, 2*(int)grid::NUM_JOINTS, d_df_du, N);
    if (!rc && N > 0 && (!d_qdd || !d_Minv)) rc = fail_msg(hipErrorInvalidValue, "null qdd or Minv pointer");
    device_launch<T> L(h, N, shape::GENERAL, rc);
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::forward_dynamics_gradient_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_df_du, d_q_qd, stride, d_qdd, d_Minv, L.model, gravity, N);
    return launch_status();
}

template <typename T>
static int id_device(grid_handle *h, const T *d_q_qd, int stride, const T *d_qdd, int N, T gravity, T *d_c, void *stream) {
    device_launch<T> L(h, N, shape::ID, check_device_io(h, d_q_qd, stride, 2*(int)grid::NUM_JOINTS, d_c, N));
    if (!L.ready) return L.rc;
    if (d_qdd) {
        hipLaunchKernelGGL((grid::inverse_dynamics_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_c, d_q_qd, stride, d_qdd, L.model, gravity, N);
    } else {
        hipLaunchKernelGGL((grid::inverse_dynamics_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_c, d_q_qd, stride, L.model, gravity, N);
    }
    return launch_status();
}

template <typename T>
static int id_grad_device(grid_handle *h, const T *d_q_qd, int stride, const T *d_qdd, int N, T gravity, T *d_dc_du, void *stream) {
    device_launch<T> L(h, N, shape::ID_DU, check_device_io(h, d_q_qd, stride, 2*(int)grid::NUM_JOINTS, d_dc_du, N));
    if (!L.ready) return L.rc;
    if (d_qdd) {
        hipLaunchKernelGGL((grid::inverse_dynamics_gradient_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_dc_du, d_q_qd, stride, d_qdd, L.model, gravity, N);
    } else {
        hipLaunchKernelGGL((grid::inverse_dynamics_gradient_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_dc_du, d_q_qd, stride, L.model, gravity, N);
    }
    return launch_status();
}

template <typename T>
static int minv_device(grid_handle *h, const T *d_q, int stride, int N, T *d_Minv, void *stream) {
    device_launch<T> L(h, N, shape::MINV, check_device_io(h, d_q, stride, 1*(int)grid::NUM_JOINTS, d_Minv, N));
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::direct_minv_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_Minv, d_q, stride, L.model, N);
    return launch_status();
}

template <typename T>
static int fd_device(grid_handle *h, const T *d_q_qd_u, int stride, int N, T gravity, T *d_qdd, void *stream, bool aba) {
    device_launch<T> L(h, N, aba ? shape::ABA : shape::FD, check_device_io(h, d_q_qd_u, stride, 3*(int)grid::NUM_JOINTS, d_qdd, N));
    if (!L.ready) return L.rc;
    if (aba) {
        hipLaunchKernelGGL((grid::aba_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_qdd, d_q_qd_u, stride, L.model, gravity, N);
    } else {
        hipLaunchKernelGGL((grid::forward_dynamics_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_qdd, d_q_qd_u, stride, L.model, gravity, N);
    }
    return launch_status();
}

template <typename T>
static int idsva_so_device(grid_handle *h, const T *d_q_qd_u, int stride, const T *d_qdd, int N, T gravity, T *d_idsva_so, void *stream) {
    const int rc = check_device_io(h, d_q_qd_u, stride, 2*(int)grid::NUM_JOINTS, d_idsva_so, N);
#if GRID_HAS_IDSVA_SO
    device_launch<T> L(h, N, shape::IDSVA_SO, rc);
    if (!L.ready) return L.rc;
    const grid_so::robotModel<T> *model = reinterpret_cast<const grid_so::robotModel<T> *>(L.model);
    if (d_qdd) {
        hipLaunchKernelGGL((grid_so::idsva_so_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_idsva_so, d_q_qd_u, stride, d_qdd, model, gravity, N);
    } else {
        hipLaunchKernelGGL((grid_so::idsva_so_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_idsva_so, d_q_qd_u, stride, model, gravity, N);
    }
    return launch_status();
#else
    if (rc) return rc;
    (void)d_q_qd_u; (void)stride; (void)d_qdd; (void)gravity; (void)d_idsva_so; (void)stream;
    return fail_msg(hipErrorNotSupported, "idsva_so is not emitted for this library's robot (see GRID_HAS_IDSVA_SO in the generated header)");
#endif
}

template <typename T>
static int fdsva_so_device(grid_handle *h, const T *d_q_qd_u, int stride, int N, T gravity, T *d_df2, void *stream) {
    const int rc = check_device_io(h, d_q_qd_u, stride, 3*(int)grid::NUM_JOINTS, d_df2, N);
#if GRID_HAS_IDSVA_SO
    device_launch<T> L(h, N, shape::FDSVA_SO, rc);
    if (!L.ready) return L.rc;
    const grid_so::robotModel<T> *model = reinterpret_cast<const grid_so::robotModel<T> *>(L.model);
#if GRID_SO_DIRECT
    // the idsva_so tensors of a solve do not fit LDS: the kernel keeps them in the handle's d_idsva_so buffer
    if (N > so_capacity<T>(h)) return fail_msg(hipErrorInvalidValue, "num_timesteps exceeds the handle's second-order workspace (grid_second_order_capacity)");
    {
        std::lock_guard<std::mutex> lock(h->alloc_lock);
        if (!h->so_done) GRID_TRY(hipEventCreateWithFlags(&h->so_done, hipEventDisableTiming));
        if (h->so_pending) GRID_TRY(hipStreamWaitEvent((hipStream_t)stream, h->so_done, 0));  // (the previous launch may be on another stream)
#if GRID_SO_SPLIT
        // two kernels: gradient, M^-1 and the tensors by lane groups into the handle's buffers, then the contraction with one block per solve
        hipLaunchKernelGGL((grid_so::fdsva_so_prepare_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, typed<T>(h).hd_data->d_idsva_so, typed<T>(h).hd_data->d_df_du,
                           typed<T>(h).hd_data->d_Minv, d_q_qd_u, stride, model, gravity, N);
        GRID_TRY(hipGetLastError());
        hipLaunchKernelGGL((grid_so::fdsva_so_contract_kernel<T>), dim3(N < 4096 ? N : 4096), dim3(grid_so::FDSVA_SO_CONTRACT_THREADS), (size_t)grid_so::FDSVA_SO_CONTRACT_LDS * sizeof(T),
                           (hipStream_t)stream, d_df2, typed<T>(h).hd_data->d_idsva_so, typed<T>(h).hd_data->d_df_du, typed<T>(h).hd_data->d_Minv, N);
#else
        hipLaunchKernelGGL((grid_so::fdsva_so_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_df2, typed<T>(h).hd_data->d_idsva_so, d_q_qd_u, stride, model, gravity, N);
#endif
        GRID_TRY(hipGetLastError());
        GRID_TRY(hipEventRecord(h->so_done, (hipStream_t)stream));
        h->so_pending = true;
    }
#else
    hipLaunchKernelGGL((grid_so::fdsva_so_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_df2, d_q_qd_u, stride, model, gravity, N);
#endif
    return launch_status();
#else
    if (rc) return rc;
    (void)d_q_qd_u; (void)stride; (void)gravity; (void)d_df2; (void)stream;
    return fail_msg(hipErrorNotSupported, "fdsva_so is not emitted for this library's robot (see GRID_HAS_IDSVA_SO in the generated header)");
#endif
}

// ---------------------------------------------------------------------------------------------------------------- host entry points
// Host buffers in, host buffers out, synchronous: H2D on the handle's stream, launch, D2H, stream sync - the semantics of the
// reference's host wrappers (e.g. reference algorithms/_inverse_dynamics.py:440-512), with the handle's device buffers as staging.
template <typename T>
static int host_prologue(grid_handle *h, int N) {
    int rc = check_args(h, N);
    if (rc) return rc;
    if (N > h->max_timesteps) return fail_msg(hipErrorInvalidValue, "num_timesteps exceeds grid_init's max_timesteps");
    return 0;
}
#define GRID_H2D(dst, src, count) GRID_TRY(hipMemcpyAsync((dst), (src), (size_t)(count) * sizeof(T), hipMemcpyHostToDevice, s))
#define GRID_D2H(dst, src, count) GRID_TRY(hipMemcpyAsync((dst), (src), (size_t)(count) * sizeof(T), hipMemcpyDeviceToHost, s))

// true where `ptr` is page-locked host memory the GPU's copy engines can reach directly (hipHostMalloc / grid_host_alloc / hipHostRegister): only then is
// hipMemcpyAsync asynchronous.  (Pinning a caller's pageable buffer for one call was tried: hipHostRegister of a freshly allocated 6.4 MB result buffer costs more
// than the overlap gains - 64 instead of 77 M solves/s end to end.)
static bool is_pinned_host(const void *ptr) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// The hot path's host entry point.  Semantics of the reference's wrapper (H2D, launch, D2H, synchronous on return; reference
// algorithms/_forward_dynamics_gradient.py:221-245).  Where BOTH of the caller's buffers are page-locked (grid_host_alloc) the batch is cut into chunks that
// travel on the handle's three streams: the copy engines run H2D of chunk c+1 and D2H of chunk c-1 beside the kernel of chunk c.  Pageable buffers take the
// strictly sequential form (hipMemcpyAsync blocks on them anyway).
template <typename T>
static int fd_grad_host(grid_handle *h, const T *h_q_qd_u, int N, T gravity, T *h_df_du) {
    int rc = host_prologue<T>(h, N);
    if (rc || N == 0) return rc;
    if (!h_q_qd_u || !h_df_du) return fail_msg(hipErrorInvalidValue, "null input or output pointer");
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    const size_t n = grid::NUM_JOINTS;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    const int min_chunk = 2048;  // (below that a chunk's kernel is all launch latency)
    int chunks = N / min_chunk;
    if (chunks > 3) chunks = 3;  // (one chunk per stream; measured at 16 384 solves, page-locked buffers: 1 chunk 178 us, 2: 176, 3: 172.5, 4: 206, 8: 244 - tools/bench_host_pipeline.py)
    if (h->host_chunks > 0) chunks = h->host_chunks < N ? h->host_chunks : N;
    if (chunks < 2 || !is_pinned_host(h_q_qd_u) || !is_pinned_host(h_df_du)) {
        hipStream_t s = h->streams[0];
        GRID_H2D(d->d_q_qd_u, h_q_qd_u, 3 * n * N);
        if ((rc = fd_grad_device<T>(h, d->d_q_qd_u, 3 * (int)n, N, gravity, d->d_df_du, (void *)s))) return rc;
        GRID_D2H(h_df_du, d->d_df_du, 2 * n * n * N);
        GRID_TRY(hipStreamSynchronize(s));
        return 0;
    }
    const int per = (N + chunks - 1) / chunks;
    for (int c = 0; c < chunks; c++) {
        const int k0 = c * per, cnt = (k0 + per <= N) ? per : N - k0;
        if (cnt <= 0) break;
        hipStream_t s = h->streams[c % 3];
        hipError_t e = hipMemcpyAsync(d->d_q_qd_u + (size_t)k0 * 3 * n, h_q_qd_u + (size_t)k0 * 3 * n, 3 * n * (size_t)cnt * sizeof(T), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { rc = fail(e, "hipMemcpyAsync(H2D)"); break; }  // (no early return: the streams are drained below)
        if ((rc = fd_grad_device<T>(h, d->d_q_qd_u + (size_t)k0 * 3 * n, 3 * (int)n, cnt, gravity, d->d_df_du + (size_t)k0 * 2 * n * n, (void *)s))) break;
        e = hipMemcpyAsync(h_df_du + (size_t)k0 * 2 * n * n, d->d_df_du + (size_t)k0 * 2 * n * n, 2 * n * n * (size_t)cnt * sizeof(T), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) { rc = fail(e, "hipMemcpyAsync(D2H)"); break; }
    }
    for (int c = 0; c < 3; c++) {  // (always drained: the call is synchronous on return)
        hipError_t e = hipStreamSynchronize(h->streams[c]);
        if (e != hipSuccess && !rc) rc = fail(e, "hipStreamSynchronize");
    }
    return rc;
}

template <typename T>
static int fd_grad_qdd_minv_host(grid_handle *h, const T *h_q_qd, int stride, const T *h_qdd, const T *h_Minv, int N, T gravity, T *h_df_du) {
    int rc = host_prologue<T>(h, N);
    if (rc || N == 0) return rc;
    const size_t n = grid::NUM_JOINTS;
    if (stride < 2 * (int)n || stride > 3 * (int)n) return fail_msg(hipErrorInvalidValue, "stride must be in [2n, 3n] for host buffers");
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_q_qd, (size_t)stride * N);
    GRID_H2D(d->d_qdd, h_qdd, n * N);
    GRID_H2D(d->d_Minv, h_Minv, n * n * N);
    if ((rc = fd_grad_qdd_minv_device<T>(h, d->d_q_qd_u, stride, d->d_qdd, d->d_Minv, N, gravity, d->d_df_du, (void *)s))) return rc;
    GRID_D2H(h_df_du, d->d_df_du, 2 * n * n * N);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

// which: 0 = inverse dynamics (c), 1 = its gradient (dc_du)
template <typename T>
static int id_host(grid_handle *h, const T *h_q_qd, int stride, const T *h_qdd, int N, T gravity, T *h_out, int which) {
    int rc = host_prologue<T>(h, N);
    if (rc || N == 0) return rc;
    const size_t n = grid::NUM_JOINTS;
    if (stride < 2 * (int)n || stride > 3 * (int)n) return fail_msg(hipErrorInvalidValue, "stride must be in [2n, 3n] for host buffers (USE_COMPRESSED_MEM: 2n)");
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_q_qd, (size_t)stride * N);
    if (h_qdd) GRID_H2D(d->d_qdd, h_qdd, n * N);
    if (which == 0) {
        if ((rc = id_device<T>(h, d->d_q_qd_u, stride, h_qdd ? d->d_qdd : nullptr, N, gravity, d->d_c, (void *)s))) return rc;
        GRID_D2H(h_out, d->d_c, n * N);
    } else {
        if ((rc = id_grad_device<T>(h, d->d_q_qd_u, stride, h_qdd ? d->d_qdd : nullptr, N, gravity, d->d_dc_du, (void *)s))) return rc;
        GRID_D2H(h_out, d->d_dc_du, 2 * n * n * N);
    }
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

template <typename T>
static int minv_host(grid_handle *h, const T *h_q, int stride, int N, T *h_Minv) {
    int rc = host_prologue<T>(h, N);
    if (rc || N == 0) return rc;
    const size_t n = grid::NUM_JOINTS;
    if (stride < (int)n || stride > 3 * (int)n) return fail_msg(hipErrorInvalidValue, "stride must be in [n, 3n] for host buffers (USE_COMPRESSED_MEM: n)");
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_q, (size_t)stride * N);
    if ((rc = minv_device<T>(h, d->d_q_qd_u, stride, N, d->d_Minv, (void *)s))) return rc;
    GRID_D2H(h_Minv, d->d_Minv, n * n * N);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

template <typename T>
static int fd_host(grid_handle *h, const T *h_q_qd_u, int N, T gravity, T *h_qdd, bool aba) {
    int rc = host_prologue<T>(h, N);
    if (rc || N == 0) return rc;
    const size_t n = grid::NUM_JOINTS;
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_q_qd_u, 3 * n * N);
    if ((rc = fd_device<T>(h, d->d_q_qd_u, 3 * (int)n, N, gravity, d->d_qdd, (void *)s, aba))) return rc;
    GRID_D2H(h_qdd, d->d_qdd, n * N);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

// which: 0 = idsva_so (h_qdd may be NULL), 1 = fdsva_so
template <typename T>
static int so_host(grid_handle *h, const T *h_q_qd_u, const T *h_qdd, int N, T gravity, T *h_out, int which) {
    int rc = host_prologue<T>(h, N);
    if (rc) return rc;
#if GRID_HAS_IDSVA_SO
    if (N == 0) return 0;
    if (N > so_capacity<T>(h)) return fail_msg(hipErrorInvalidValue, "num_timesteps exceeds the handle's second-order buffers (grid_second_order_capacity)");
    const size_t n = grid::NUM_JOINTS;
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_q_qd_u, 3 * n * N);
    if (which == 0) {
        if (h_qdd) GRID_H2D(d->d_qdd, h_qdd, n * N);
        if ((rc = idsva_so_device<T>(h, d->d_q_qd_u, 3 * (int)n, h_qdd ? d->d_qdd : nullptr, N, gravity, d->d_idsva_so, (void *)s))) return rc;
        GRID_D2H(h_out, d->d_idsva_so, 4 * n * n * n * N);
    } else {
        if ((rc = fdsva_so_device<T>(h, d->d_q_qd_u, 3 * (int)n, N, gravity, d->d_df2, (void *)s))) return rc;
        GRID_D2H(h_out, d->d_df2, 4 * n * n * n * N);
    }
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
#else
    (void)h_q_qd_u; (void)h_qdd; (void)gravity; (void)h_out; (void)which;
    return fail_msg(hipErrorNotSupported, "the second-order kernels are not emitted for this library's robot (see GRID_HAS_IDSVA_SO in the generated header)");
#endif
}

// ---------------------------------------------------------------------------------------------------------------- end-effector kinematics
// which: 0 = pose (d_out = eePos, 6E per solve), 1 = gradient (deePos, 6En), 2 = Hessian (d2eePos, 6En^2; d_dee receives the gradient or is NULL)
static const size_t EE_REC[3] = {(size_t)6 * grid::NUM_EES, (size_t)6 * grid::NUM_EES * grid::NUM_JOINTS, (size_t)6 * grid::NUM_EES * grid::NUM_JOINTS * grid::NUM_JOINTS};

template <typename T>
static int ee_device(grid_handle *h, const T *d_q, int stride, int N, T *d_out, T *d_dee, void *stream, int which) {
    device_launch<T> L(h, N, shape::EE[which], check_device_io(h, d_q, stride, (int)grid::NUM_JOINTS, d_out, N));
    if (!L.ready) return L.rc;
    if (which == 0) {
        hipLaunchKernelGGL((grid::end_effector_pose_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_out, d_q, stride, L.model, N);
    } else if (which == 1) {
        hipLaunchKernelGGL((grid::end_effector_pose_gradient_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_out, d_q, stride, L.model, N);
    } else {
        hipLaunchKernelGGL((grid::end_effector_pose_gradient_hessian_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_out, d_dee, d_q, stride, L.model, N);
    }
    return launch_status();
}

// grows one device staging buffer to at least `count` elements (the caller holds alloc_lock)
template <typename T>
static int grow_staging(T **buf, size_t *cap, size_t count) {
    if (*cap >= count) return 0;
    if (*buf) GRID_TRY(hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    GRID_TRY(hipMalloc((void **)buf, count * sizeof(T)));
    *cap = count;
    return 0;
}

// Host buffers in, host buffers out, synchronous.  The handle's kinematics staging is allocated here on first use; the Hessian's holds at most
// 1 GiB (like the second-order buffers) and longer batches pass through it in chunks.
template <typename T>
static int ee_host(grid_handle *h, const T *h_q, int stride, int N, T *h_out, T *h_dee, int which) {
    int rc = host_prologue<T>(h, N);
    if (rc || N == 0) return rc;
    if (!h_q || !h_out) return fail_msg(hipErrorInvalidValue, "null input or output pointer");
    if (stride < (int)grid::NUM_JOINTS) {
        snprintf(g_err, sizeof(g_err), "stride %d is smaller than the %d joint positions of a solve", stride, (int)grid::NUM_JOINTS);
        return (int)hipErrorInvalidValue;
    }
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    const size_t rec = EE_REC[which], grad = EE_REC[1];
    const bool dee = which == 2 && h_dee != nullptr;
    size_t chunk = (size_t)N;
    const size_t cap = ((size_t)1 << 30) / (rec * sizeof(T));
    if (chunk > cap) chunk = cap > 0 ? cap : 1;
    ee_stage<T> &st = ee_staging<T>(h);
    {
        std::lock_guard<std::mutex> lock(h->alloc_lock);
        if ((rc = grow_staging<T>(&st.d_q, &st.q_cap, (size_t)stride * chunk))) return rc;
        if ((rc = grow_staging<T>(&st.d_out, &st.out_cap, rec * chunk))) return rc;
        if (dee && (rc = grow_staging<T>(&st.d_dee, &st.dee_cap, grad * chunk))) return rc;
    }
    hipStream_t s = h->streams[0];
    for (size_t k0 = 0; k0 < (size_t)N; k0 += chunk) {
        const size_t cnt = (k0 + chunk <= (size_t)N) ? chunk : (size_t)N - k0;
        GRID_H2D(st.d_q, h_q + k0 * stride, (size_t)stride * cnt);
        if ((rc = ee_device<T>(h, st.d_q, stride, (int)cnt, st.d_out, dee ? st.d_dee : nullptr, (void *)s, which))) return rc;
        GRID_D2H(h_out + k0 * rec, st.d_out, rec * cnt);
        if (dee) GRID_D2H(h_dee + k0 * grad, st.d_dee, grad * cnt);
    }
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

template <typename T>
static void ee_release(ee_stage<T> &st) {
    if (st.d_q) (void)hipFree(st.d_q);
    if (st.d_out) (void)hipFree(st.d_out);
    if (st.d_dee) (void)hipFree(st.d_dee);
    st = ee_stage<T>();
}

// ---------------------------------------------------------------------------------------------------------------- joint-space inertia matrix
template <typename T>
static int crba_device(grid_handle *h, const T *d_q, int stride, int N, T *d_M, void *stream) {
    device_launch<T> L(h, N, shape::CRBA, check_device_io(h, d_q, stride, (int)grid::NUM_JOINTS, d_M, N));
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::crba_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_M, d_q, stride, L.model, (T)0, N);
    return launch_status();
}

// Host buffers in, host buffers out, synchronous.  The output is staged in the handle's own hd_data->d_M (null after init_gridData, allocated here on
// first use and grown by longer calls, freed by close_grid) - no other entry point's buffer is borrowed, and no pinned h_M is allocated (the result
// goes straight to the caller's buffer).
template <typename T>
static int crba_host(grid_handle *h, const T *h_q, int stride, int N, T *h_M) {
    int rc = host_prologue<T>(h, N);
    if (rc || N == 0) return rc;
    if (!h_q || !h_M) return fail_msg(hipErrorInvalidValue, "null input or output pointer");
    const size_t n = grid::NUM_JOINTS;
    if (stride < (int)n || stride > 3 * (int)n) return fail_msg(hipErrorInvalidValue, "stride must be in [n, 3n] for host buffers (USE_COMPRESSED_MEM: 2n)");
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    {
        std::lock_guard<std::mutex> lock(h->alloc_lock);
        if ((rc = grow_staging<T>(&d->d_M, &typed<T>(h).M_cap, n * n * (size_t)N))) return rc;
    }
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_q, (size_t)stride * N);
    if ((rc = crba_device<T>(h, d->d_q_qd_u, stride, N, d->d_M, (void *)s))) return rc;
    GRID_D2H(h_M, d->d_M, n * n * N);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- fused rollout
// u: element (t, k, j) at d_u[t*stride_u_step + k*stride_u_solve + j].  Every solve's row must lie inside its step and the steps must not overlap
// (a smaller or negative stride would read before / past the caller's buffer); stride_u_solve == 0 is the one legal alias: one sequence for all solves.
static long rollout_u_span(int stride_u_solve, int N) {  // what one step of the control touches
    const long n = grid::NUM_JOINTS;
    return stride_u_solve == 0 ? n : (long)(N - 1) * stride_u_solve + n;
}

// The checks every rollout entry point makes after check_args / host_prologue.  have_inputs, have_outputs: the caller's own null tests, the texts what it says
// where they fail.  N == 0 is legal whatever the pointers are: 0 is returned before they are looked at, and the caller returns.
static int check_rollout_call(int N, int num_steps, bool have_inputs, const char *no_inputs, bool have_outputs, const char *no_outputs, int stride_x0, long stride_u_step,
                              int stride_u_solve) {
    if (num_steps < 0) return fail_msg(hipErrorInvalidValue, "negative num_steps");
    if (N == 0) return 0;
    if (!have_inputs) return fail_msg(hipErrorInvalidValue, no_inputs);
    if (!have_outputs) return fail_msg(hipErrorInvalidValue, no_outputs);
    const int n = (int)grid::NUM_JOINTS;
    if (stride_x0 < 2 * n) {
        snprintf(g_err, sizeof(g_err), "stride_x0 %d is smaller than the %d values [q | qd] the kernel reads per solve", stride_x0, 2 * n);
        return (int)hipErrorInvalidValue;
    }
    if (stride_u_solve != 0 && stride_u_solve < n) {
        snprintf(g_err, sizeof(g_err), "stride_u_solve %d must be 0 (one control sequence for all solves) or at least the %d controls of a solve", stride_u_solve, n);
        return (int)hipErrorInvalidValue;
    }
    const long span = rollout_u_span(stride_u_solve, N);
    if (span > (long)INT_MAX) return fail_msg(hipErrorInvalidValue, "stride_u_solve * num_solves exceeds the 32-bit offsets the kernel uses inside one step");
    if (num_steps > 1 && stride_u_step < span) {
        snprintf(g_err, sizeof(g_err), "stride_u_step %ld is smaller than the %ld values one step of the control spans", stride_u_step, span);
        return (int)hipErrorInvalidValue;
    }
    return 0;
}

// elements of the records the host entry points stage: the control as the caller laid it out ((num_steps - 1) whole steps and the span of the last one), one
// (N, 2n) row of states, the num_steps + 1 rows of a trajectory
struct rollout_counts {
    size_t u, row, traj;
};
static rollout_counts rollout_extent(long stride_u_step, int stride_u_solve, int N, int num_steps) {
    rollout_counts e;
    e.u = num_steps > 0 ? (size_t)(num_steps - 1) * (size_t)stride_u_step + (size_t)rollout_u_span(stride_u_solve, N) : 0;
    e.row = 2 * (size_t)grid::NUM_JOINTS * (size_t)N;
    e.traj = e.row * ((size_t)num_steps + 1);
    return e;
}

// the states of a forward rollout inside the handle's d_x_traj: the trajectory where it is asked for, xT behind it (alone: at the front)
struct rollout_x_layout {
    size_t count, xT_offset;
    rollout_x_layout(const rollout_counts &e, bool traj, bool xT) : count(traj ? e.traj + (xT ? e.row : 0) : e.row), xT_offset(traj ? e.traj : 0) {}
};

// No staged record of a host call may exceed GRID_ROLLOUT_LIN_HOST_CAP_BYTES: such a call is refused before anything is allocated or copied.
static int check_rollout_staging(const char *entry, int N, int num_steps, std::initializer_list<size_t> counts, size_t elem_bytes) {
    const size_t largest = std::max(counts);
    if (largest <= GRID_ROLLOUT_LIN_HOST_CAP_BYTES / elem_bytes) return 0;
    snprintf(g_err, sizeof(g_err), "%s host staging capacity exceeded: %d solves x %d steps need %zu bytes for the largest record, the cap is %zu "
             "(split the horizon or use the device entry point)", entry, N, num_steps, largest * elem_bytes, (size_t)GRID_ROLLOUT_LIN_HOST_CAP_BYTES);
    return (int)hipErrorInvalidValue;
}

template <typename T>
static int rollout_device(grid_handle *h, const T *d_x0, int stride_x0, const T *d_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                          T *d_traj, T *d_xT, void *stream) {
    int rc = check_args(h, N);
    if (!rc) rc = check_rollout_call(N, num_steps, d_x0 && (num_steps == 0 || d_u), "null input pointer", d_traj || d_xT,
                                     "null output pointers: at least one of traj and xT must be given", stride_x0, stride_u_step, stride_u_solve);
    device_launch<T> L(h, N, shape::ROLLOUT, rc);
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::rollout_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_traj, d_xT, d_x0, stride_x0, d_u, stride_u_step, stride_u_solve,
                       L.model, dt, gravity, N, num_steps);
    return launch_status();
}

// Host buffers in, host buffers out, synchronous.  x0 passes through the handle's d_q_qd_u; u and traj / xT do not fit the handle's 3n-per-solve buffers:
// they are staged in hd_data->d_u_traj / d_x_traj (null after init_gridData, allocated here on first use, grown by longer calls, freed by close_grid).
template <typename T>
static int rollout_host(grid_handle *h, const T *h_x0, int stride_x0, const T *h_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                        T *h_traj, T *h_xT) {
    int rc = host_prologue<T>(h, N);
    if (!rc) rc = check_rollout_call(N, num_steps, h_x0 && (num_steps == 0 || h_u), "null input pointer", h_traj || h_xT,
                                     "null output pointers: at least one of traj and xT must be given", stride_x0, stride_u_step, stride_u_solve);
    if (rc || N == 0) return rc;
    if (stride_x0 > 3 * (int)grid::NUM_JOINTS) return fail_msg(hipErrorInvalidValue, "stride_x0 must be in [2n, 3n] for host buffers");
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    const rollout_counts e = rollout_extent(stride_u_step, stride_u_solve, N, num_steps);
    const rollout_x_layout x(e, h_traj, h_xT);
    {
        std::lock_guard<std::mutex> lock(h->alloc_lock);
        if ((rc = grow_staging<T>(&d->d_u_traj, &typed<T>(h).u_traj_cap, e.u > 0 ? e.u : 1))) return rc;
        if ((rc = grow_staging<T>(&d->d_x_traj, &typed<T>(h).x_traj_cap, x.count))) return rc;
    }
    T *d_traj = h_traj ? d->d_x_traj : nullptr, *d_xT = h_xT ? d->d_x_traj + x.xT_offset : nullptr;
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_x0, (size_t)stride_x0 * N);
    if (e.u > 0) GRID_H2D(d->d_u_traj, h_u, e.u);
    if ((rc = rollout_device<T>(h, d->d_q_qd_u, stride_x0, d->d_u_traj, stride_u_step, stride_u_solve, N, num_steps, dt, gravity, d_traj, d_xT, (void *)s))) return rc;
    if (h_traj) GRID_D2H(h_traj, d_traj, e.traj);
    if (h_xT) GRID_D2H(h_xT, d_xT, e.row);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- linearised rollout
// The rollout above plus, per step, the Jacobian records fx (2n^2) and fu (n^2).  Same validation; at least one of the four outputs must be given.
template <typename T>
static int rollout_linearized_device(grid_handle *h, const T *d_x0, int stride_x0, const T *d_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                                     T *d_traj, T *d_xT, T *d_fx, T *d_fu, void *stream) {
    int rc = check_args(h, N);
    if (!rc) rc = check_rollout_call(N, num_steps, d_x0 && (num_steps == 0 || d_u), "null input pointer", d_traj || d_xT || d_fx || d_fu,
                                     "null output pointers: at least one of traj, xT, fx and fu must be given", stride_x0, stride_u_step, stride_u_solve);
    if (!rc && num_steps == 0 && !d_traj && !d_xT) return 0;  // (no step: no Jacobian is written)
    device_launch<T> L(h, N, shape::ROLLOUT_LIN, rc);
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::rollout_linearized_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_traj, d_xT, d_fx, d_fu, d_x0, stride_x0, d_u, stride_u_step,
                       stride_u_solve, L.model, dt, gravity, N, num_steps);
    return launch_status();
}

// Host buffers in, host buffers out, synchronous.  x0, u and traj / xT as in rollout_host, the Jacobians through hd_data->d_fx_traj / d_fu_traj (same rules).
// Subject to check_rollout_staging.
template <typename T>
static int rollout_linearized_host(grid_handle *h, const T *h_x0, int stride_x0, const T *h_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                                   T *h_traj, T *h_xT, T *h_fx, T *h_fu) {
    int rc = host_prologue<T>(h, N);
    if (!rc) rc = check_rollout_call(N, num_steps, h_x0 && (num_steps == 0 || h_u), "null input pointer", h_traj || h_xT || h_fx || h_fu,
                                     "null output pointers: at least one of traj, xT, fx and fu must be given", stride_x0, stride_u_step, stride_u_solve);
    if (rc || N == 0) return rc;
    const size_t n = grid::NUM_JOINTS;
    if (stride_x0 > 3 * (int)n) return fail_msg(hipErrorInvalidValue, "stride_x0 must be in [2n, 3n] for host buffers");
    const rollout_counts e = rollout_extent(stride_u_step, stride_u_solve, N, num_steps);
    const rollout_x_layout x(e, h_traj, h_xT);
    const size_t fx_count = h_fx ? 2 * n * n * (size_t)N * (size_t)num_steps : 0;
    const size_t fu_count = h_fu ? n * n * (size_t)N * (size_t)num_steps : 0;
    if ((rc = check_rollout_staging("rollout_linearized", N, num_steps, {fx_count, fu_count, x.count, e.u}, sizeof(T)))) return rc;
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    {
        std::lock_guard<std::mutex> lock(h->alloc_lock);
        if ((rc = grow_staging<T>(&d->d_u_traj, &typed<T>(h).u_traj_cap, e.u > 0 ? e.u : 1))) return rc;
        if ((rc = grow_staging<T>(&d->d_x_traj, &typed<T>(h).x_traj_cap, x.count))) return rc;
        if (fx_count > 0 && (rc = grow_staging<T>(&d->d_fx_traj, &typed<T>(h).fx_traj_cap, fx_count))) return rc;
        if (fu_count > 0 && (rc = grow_staging<T>(&d->d_fu_traj, &typed<T>(h).fu_traj_cap, fu_count))) return rc;
    }
    T *d_traj = h_traj ? d->d_x_traj : nullptr, *d_xT = h_xT ? d->d_x_traj + x.xT_offset : nullptr;
    T *d_fx = fx_count > 0 ? d->d_fx_traj : nullptr, *d_fu = fu_count > 0 ? d->d_fu_traj : nullptr;
    if (!d_traj && !d_xT && !d_fx && !d_fu) return 0;  // (num_steps == 0 and Jacobians only: there is nothing to write)
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_x0, (size_t)stride_x0 * N);
    if (e.u > 0) GRID_H2D(d->d_u_traj, h_u, e.u);
    if ((rc = rollout_linearized_device<T>(h, d->d_q_qd_u, stride_x0, d->d_u_traj, stride_u_step, stride_u_solve, N, num_steps, dt, gravity, d_traj, d_xT, d_fx, d_fu, (void *)s))) return rc;
    if (h_traj) GRID_D2H(h_traj, d_traj, e.traj);
    if (h_xT) GRID_D2H(h_xT, d_xT, e.row);
    if (d_fx) GRID_D2H(h_fx, d_fx, fx_count);
    if (d_fu) GRID_D2H(h_fu, d_fu, fu_count);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- rollout adjoint
// The reverse pass over a stored trajectory: grad_x0 and grad_u of a cost whose gradient with respect to the states is gx (every step) and / or gxT (the final state).
template <typename T>
static int rollout_adjoint_check(const T *traj, const T *u, long stride_u_step, int stride_u_solve, int N, int num_steps, const T *gx, const T *gxT, const T *grad_x0, const T *grad_u) {
    const int n = (int)grid::NUM_JOINTS;
    const int rc = check_rollout_call(N, num_steps, num_steps == 0 || (traj && u), "null input pointer: traj and u must be given", grad_x0 || grad_u,
                                      "null output pointers: at least one of grad_x0 and grad_u must be given", 2 * n, stride_u_step, stride_u_solve);
    if (rc || N == 0) return rc;
    if (!gx && !gxT) return fail_msg(hipErrorInvalidValue, "null cotangents: at least one of gx and gxT must be given");
    if ((long)N * 2 * n > (long)INT_MAX) return fail_msg(hipErrorInvalidValue, "2n * num_solves exceeds the 32-bit offsets the kernel uses inside one step");
    return 0;
}

template <typename T>
static int rollout_adjoint_device(grid_handle *h, const T *d_traj, const T *d_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                                  const T *d_gx, const T *d_gxT, T *d_grad_x0, T *d_grad_u, void *stream) {
    int rc = check_args(h, N);
    if (!rc) rc = rollout_adjoint_check<T>(d_traj, d_u, stride_u_step, stride_u_solve, N, num_steps, d_gx, d_gxT, d_grad_x0, d_grad_u);
    if (!rc && num_steps == 0 && !d_grad_x0) return 0;  // (no step: no grad_u is written)
    device_launch<T> L(h, N, shape::ROLLOUT_ADJ, rc);
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::rollout_adjoint_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_grad_x0, num_steps > 0 ? d_grad_u : static_cast<T *>(nullptr), d_traj, d_u,
                       stride_u_step, stride_u_solve, d_gx, d_gxT, L.model, dt, gravity, N, num_steps);
    return launch_status();
}

// Host buffers in, host buffers out, synchronous.  traj and u pass through the handle's d_x_traj / d_u_traj like rollout_host, gx, gxT and the two gradients through
// hd_data->d_gx_traj / d_gx0 / d_gu_traj (same rules; gxT rides behind gx).  Subject to check_rollout_staging.
template <typename T>
static int rollout_adjoint_host(grid_handle *h, const T *h_traj, const T *h_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                                const T *h_gx, const T *h_gxT, T *h_grad_x0, T *h_grad_u) {
    int rc = host_prologue<T>(h, N);
    if (!rc) rc = rollout_adjoint_check<T>(h_traj, h_u, stride_u_step, stride_u_solve, N, num_steps, h_gx, h_gxT, h_grad_x0, h_grad_u);
    if (rc || N == 0) return rc;
    const rollout_counts e = rollout_extent(stride_u_step, stride_u_solve, N, num_steps);
    const size_t gx_count = (h_gx ? e.traj : 0) + (h_gxT ? e.row : 0);
    const size_t gu_count = h_grad_u ? (size_t)grid::NUM_JOINTS * (size_t)N * (size_t)num_steps : 0;
    if ((rc = check_rollout_staging("rollout_adjoint", N, num_steps, {e.traj, gx_count, e.u}, sizeof(T)))) return rc;
    if (num_steps == 0 && !h_grad_x0) return 0;
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid::gridData<T> *d = typed<T>(h).hd_data;
    {
        std::lock_guard<std::mutex> lock(h->alloc_lock);
        if ((rc = grow_staging<T>(&d->d_u_traj, &typed<T>(h).u_traj_cap, e.u > 0 ? e.u : 1))) return rc;
        if ((rc = grow_staging<T>(&d->d_x_traj, &typed<T>(h).x_traj_cap, e.traj))) return rc;
        if ((rc = grow_staging<T>(&d->d_gx_traj, &typed<T>(h).gx_traj_cap, gx_count))) return rc;
        if (gu_count > 0 && (rc = grow_staging<T>(&d->d_gu_traj, &typed<T>(h).gu_traj_cap, gu_count))) return rc;
        if (h_grad_x0 && (rc = grow_staging<T>(&d->d_gx0, &typed<T>(h).gx0_cap, e.row))) return rc;
    }
    T *d_gx = h_gx ? d->d_gx_traj : nullptr, *d_gxT = h_gxT ? d->d_gx_traj + (h_gx ? e.traj : 0) : nullptr;
    T *d_grad_x0 = h_grad_x0 ? d->d_gx0 : nullptr, *d_grad_u = gu_count > 0 ? d->d_gu_traj : nullptr;
    hipStream_t s = h->streams[0];
    if (num_steps > 0) GRID_H2D(d->d_x_traj, h_traj, e.row * (size_t)num_steps);  // (row num_steps of traj is not read)
    if (e.u > 0) GRID_H2D(d->d_u_traj, h_u, e.u);
    if (h_gx) GRID_H2D(d_gx, h_gx, e.traj);
    if (h_gxT) GRID_H2D(d_gxT, h_gxT, e.row);
    if ((rc = rollout_adjoint_device<T>(h, d->d_x_traj, d->d_u_traj, stride_u_step, stride_u_solve, N, num_steps, dt, gravity, d_gx, d_gxT, d_grad_x0, d_grad_u, (void *)s))) return rc;
    if (d_grad_x0) GRID_D2H(h_grad_x0, d_grad_x0, e.row);
    if (d_grad_u) GRID_D2H(h_grad_u, d_grad_u, gu_count);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- closed-loop rollout
// The rollout above with u_t = clamp(u_ff_t + K_t (x_t - x_ref_t)) formed inside the step loop.  K and x_ref are strided records: element (t, k, i) at
// p[t*stride_step + k*stride_solve + i], i < rec.  A solve stride of 0 shares one record between the solves, a step stride of 0 between the steps; otherwise the
// records of a step must not overlap and the steps must not either (a smaller or negative stride would read before / past the caller's buffer).
static long feedback_span(long stride_solve, int N, long rec) {  // what one step of a strided record touches
    return stride_solve == 0 ? rec : (long)(N - 1) * stride_solve + rec;
}
static int check_feedback_strides(const char *what, long rec, long stride_step, long stride_solve, int N, int num_steps) {
    if (stride_step < 0 || stride_solve < 0) {
        snprintf(g_err, sizeof(g_err), "negative stride of %s: stride_%s_step %ld, stride_%s_solve %ld", what, what, stride_step, what, stride_solve);
        return (int)hipErrorInvalidValue;
    }
    if (stride_solve != 0 && stride_solve < rec) {
        snprintf(g_err, sizeof(g_err), "stride_%s_solve %ld must be 0 (one record for all solves) or at least the %ld values of a record", what, stride_solve, rec);
        return (int)hipErrorInvalidValue;
    }
    if (stride_solve > (long)INT_MAX || feedback_span(stride_solve, N, rec) > (long)INT_MAX) {
        snprintf(g_err, sizeof(g_err), "stride_%s_solve * num_solves exceeds the 32-bit offsets the kernel uses inside one step", what);
        return (int)hipErrorInvalidValue;
    }
    if (num_steps > 1 && stride_step != 0 && stride_step < feedback_span(stride_solve, N, rec)) {
        snprintf(g_err, sizeof(g_err), "stride_%s_step %ld must be 0 (one record for all steps) or at least the %ld values one step spans", what, stride_step,
                 feedback_span(stride_solve, N, rec));
        return (int)hipErrorInvalidValue;
    }
    return 0;
}
static size_t feedback_extent(long rec, long stride_step, long stride_solve, int N, int num_steps) {  // elements the kernel may read
    return num_steps > 0 ? (size_t)(num_steps - 1) * (size_t)stride_step + (size_t)feedback_span(stride_solve, N, rec) : 0;
}

// what both forms check after check_args / host_prologue; N == 0 is legal whatever the pointers are
template <typename T>
static int rollout_feedback_check(const T *x0, int stride_x0, const T *u_ff, long stride_u_step, int stride_u_solve, int N, int num_steps, const T *K, long stride_K_step,
                                  long stride_K_solve, const T *x_ref, long stride_xref_step, long stride_xref_solve, const T *u_min, const T *u_max, const T *traj,
                                  const T *xT, const T *u_out) {
    const long n = grid::NUM_JOINTS;
    int rc = check_rollout_call(N, num_steps, x0 && (num_steps == 0 || u_ff), "null input pointer", traj || xT || u_out,
                                "null output pointers: at least one of traj, xT and u_out must be given", stride_x0, stride_u_step, stride_u_solve);
    if (rc || N == 0) return rc;
    if (num_steps > 0 && (!K || !x_ref)) return fail_msg(hipErrorInvalidValue, "null input pointer: K and x_ref must be given");
    if ((u_min == nullptr) != (u_max == nullptr)) return fail_msg(hipErrorInvalidValue, "torque limits: u_min and u_max must be given together, or both be NULL");
    if ((rc = check_feedback_strides("K", 2 * n * n, stride_K_step, stride_K_solve, N, num_steps))) return rc;
    return check_feedback_strides("xref", 2 * n, stride_xref_step, stride_xref_solve, N, num_steps);
}

template <typename T>
static int rollout_feedback_device(grid_handle *h, const T *d_x0, int stride_x0, const T *d_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                                   const T *d_K, long stride_K_step, long stride_K_solve, const T *d_xref, long stride_xref_step, long stride_xref_solve, const T *d_u_min,
                                   const T *d_u_max, T *d_traj, T *d_xT, T *d_u_out, void *stream) {
    int rc = check_args(h, N);
    if (!rc) rc = rollout_feedback_check<T>(d_x0, stride_x0, d_u, stride_u_step, stride_u_solve, N, num_steps, d_K, stride_K_step, stride_K_solve, d_xref, stride_xref_step,
                                            stride_xref_solve, d_u_min, d_u_max, d_traj, d_xT, d_u_out);
    if (!rc && num_steps == 0 && !d_traj && !d_xT) return 0;  // (no step: no control is written)
    device_launch<T> L(h, N, shape::ROLLOUT_FB, rc);
    if (!L.ready) return L.rc;
    hipLaunchKernelGGL((grid::rollout_feedback_kernel<T>), L.grid, L.block, L.lds, (hipStream_t)stream, d_traj, d_xT, num_steps > 0 ? d_u_out : static_cast<T *>(nullptr), d_x0,
                       stride_x0, d_u, stride_u_step, stride_u_solve, d_K, stride_K_step, (int)stride_K_solve, d_xref, stride_xref_step, (int)stride_xref_solve, d_u_min, d_u_max,
                       L.model, dt, gravity, N, num_steps);
    return launch_status();
}

// Host buffers in, host buffers out, synchronous.  x0, u_ff and traj / xT as in rollout_host; K, x_ref, the limits and u_out pass through hd_data->d_K_traj /
// d_xref_traj / d_u_lim / d_uout_traj (same rules).  K and x_ref are staged as the caller laid them out: a shared or time-invariant record is copied once.
// Subject to check_rollout_staging.
template <typename T>
static int rollout_feedback_host(grid_handle *h, const T *h_x0, int stride_x0, const T *h_u, long stride_u_step, int stride_u_solve, int N, int num_steps, T dt, T gravity,
                                 const T *h_K, long stride_K_step, long stride_K_solve, const T *h_xref, long stride_xref_step, long stride_xref_solve, const T *h_u_min,
                                 const T *h_u_max, T *h_traj, T *h_xT, T *h_u_out) {
    int rc = host_prologue<T>(h, N);
    if (!rc) rc = rollout_feedback_check<T>(h_x0, stride_x0, h_u, stride_u_step, stride_u_solve, N, num_steps, h_K, stride_K_step, stride_K_solve, h_xref, stride_xref_step,
                                            stride_xref_solve, h_u_min, h_u_max, h_traj, h_xT, h_u_out);
    if (rc || N == 0) return rc;
    const size_t n = grid::NUM_JOINTS;
    if (stride_x0 > 3 * (int)n) return fail_msg(hipErrorInvalidValue, "stride_x0 must be in [2n, 3n] for host buffers");
    const rollout_counts e = rollout_extent(stride_u_step, stride_u_solve, N, num_steps);
    const rollout_x_layout x(e, h_traj, h_xT);
    const size_t K_count = feedback_extent(2 * (long)(n * n), stride_K_step, stride_K_solve, N, num_steps);
    const size_t xref_count = feedback_extent(2 * (long)n, stride_xref_step, stride_xref_solve, N, num_steps);
    const size_t uout_count = h_u_out ? n * (size_t)N * (size_t)num_steps : 0;
    if ((rc = check_rollout_staging("rollout_feedback", N, num_steps, {K_count, xref_count, uout_count, x.count, e.u}, sizeof(T)))) return rc;
    if (num_steps == 0 && !h_traj && !h_xT) return 0;  // (no step: no control is written)
    GRID_ON_DEVICE(h);
    if ((rc = ensure_typed<T>(h))) return rc;
    grid_typed<T> &t = typed<T>(h);
    grid::gridData<T> *d = t.hd_data;
    const bool limits = h_u_min != nullptr;
    {
        std::lock_guard<std::mutex> lock(h->alloc_lock);
        if ((rc = grow_staging<T>(&d->d_u_traj, &t.u_traj_cap, e.u > 0 ? e.u : 1))) return rc;
        if ((rc = grow_staging<T>(&d->d_x_traj, &t.x_traj_cap, x.count))) return rc;
        if (K_count > 0 && (rc = grow_staging<T>(&d->d_K_traj, &t.K_traj_cap, K_count))) return rc;
        if (xref_count > 0 && (rc = grow_staging<T>(&d->d_xref_traj, &t.xref_traj_cap, xref_count))) return rc;
        if (uout_count > 0 && (rc = grow_staging<T>(&d->d_uout_traj, &t.uout_traj_cap, uout_count))) return rc;
        if (limits && (rc = grow_staging<T>(&d->d_u_lim, &t.u_lim_cap, 2 * n))) return rc;
    }
    T *d_traj = h_traj ? d->d_x_traj : nullptr, *d_xT = h_xT ? d->d_x_traj + x.xT_offset : nullptr, *d_u_out = uout_count > 0 ? d->d_uout_traj : nullptr;
    hipStream_t s = h->streams[0];
    GRID_H2D(d->d_q_qd_u, h_x0, (size_t)stride_x0 * N);
    if (e.u > 0) GRID_H2D(d->d_u_traj, h_u, e.u);
    if (K_count > 0) GRID_H2D(d->d_K_traj, h_K, K_count);
    if (xref_count > 0) GRID_H2D(d->d_xref_traj, h_xref, xref_count);
    if (limits) {
        GRID_H2D(d->d_u_lim, h_u_min, n);
        GRID_H2D(d->d_u_lim + n, h_u_max, n);
    }
    if ((rc = rollout_feedback_device<T>(h, d->d_q_qd_u, stride_x0, d->d_u_traj, stride_u_step, stride_u_solve, N, num_steps, dt, gravity, d->d_K_traj, stride_K_step,
                                         stride_K_solve, d->d_xref_traj, stride_xref_step, stride_xref_solve, limits ? d->d_u_lim : nullptr, limits ? d->d_u_lim + n : nullptr,
                                         d_traj, d_xT, d_u_out, (void *)s)))
        return rc;
    if (h_traj) GRID_D2H(h_traj, d_traj, e.traj);
    if (h_xT) GRID_D2H(h_xT, d_xT, e.row);
    if (d_u_out) GRID_D2H(h_u_out, d_u_out, uout_count);
    GRID_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- multi-GPU driver
// One process, G handles (one per GPU): the batch [0, N) is cut into G contiguous ranges of ceil(N/G) solves (SURVEY.md section 8(e),
// 16 384 total -> 16 384/G per GPU, no collective).  Every device has its own robotModel copy and stream.
static inline void multi_range(int N, int G, int g, int *k0, int *cnt) {
    const int per = (N + G - 1) / G;
    int a = g * per, b = a + per;
    if (a > N) a = N;
    if (b > N) b = N;
    *k0 = a;
    *cnt = b - a;
}

template <typename T>
static int fd_grad_multi_host(grid_handle **hs, int G, const T *h_q_qd_u, int N, T gravity, T *h_df_du) {
    if (!hs || G < 1 || N < 0) return fail_msg(hipErrorInvalidValue, "grid_forward_dynamics_gradient_multi_host: bad arguments");
    const size_t n = grid::NUM_JOINTS;
    std::vector<int> rcs(G, 0);
    std::vector<std::string> msgs(G);
    std::vector<std::thread> ts;
    // one host thread per device: pageable host memory makes hipMemcpyAsync block, threads keep the G copy engines busy at once
    for (int g = 0; g < G; g++) {
        ts.emplace_back([&, g]() {
            int k0, cnt;
            multi_range(N, G, g, &k0, &cnt);
            rcs[g] = fd_grad_host<T>(hs[g], h_q_qd_u + (size_t)k0 * 3 * n, cnt, gravity, h_df_du + (size_t)k0 * 2 * n * n);
            if (rcs[g]) msgs[g] = g_err;  // (g_err is thread-local)
        });
    }
    for (auto &t : ts) t.join();
    for (int g = 0; g < G; g++)
        if (rcs[g]) {
            snprintf(g_err, sizeof(g_err), "device slot %d: %s", g, msgs[g].c_str());
            return rcs[g];
        }
    return 0;
}

extern "C" {

int grid_num_joints(void) { return grid::NUM_JOINTS; }
const char *grid_robot_name(void) { return GRID_ROBOT_NAME; }
int grid_lanes_per_solve(void) { return grid::GRID_LANES_PER_SOLVE; }
int grid_suggested_threads(void) { return grid::SUGGESTED_THREADS; }
int grid_lds_bytes_per_block(void) {  // what a default forward_dynamics_gradient launch asks for (same arithmetic as make_launch)
    grid_handle h{};
    launch_cfg c;
    if (make_launch<float>(&h, 1, shape::FD_DU, &c)) return -1;
    return (int)c.lds;
}
int grid_has_second_order(void) { return GRID_HAS_IDSVA_SO; }
int grid_second_order_capacity(const grid_handle *h, int f64) { return h ? (f64 ? so_capacity<double>(h) : so_capacity<float>(h)) : 0; }
const char *grid_last_error(void) { return g_err; }

int grid_init(int device, int max_timesteps, grid_handle **out) {
    if (!out || max_timesteps < 1) return fail_msg(hipErrorInvalidValue, "grid_init: bad arguments");
    *out = nullptr;
    device_guard guard(device);
    if (guard.err != hipSuccess) return fail(guard.err, "hipSetDevice(device)");
    grid_handle *h = new (std::nothrow) grid_handle();
    if (!h) return fail_msg(hipErrorOutOfMemory, "grid_init: out of host memory");
    h->device = device;
    h->max_timesteps = max_timesteps;
    h->blocks = h->threads = h->host_chunks = 0;
    h->streams = nullptr;
    int rc = 0;
    try {
        rc = ensure_typed<float>(h);
        if (!rc) h->streams = grid::init_grid<float>();
    } catch (const grid_capi_error &e) {
        snprintf(g_err, sizeof(g_err), "grid_init: %s (%s:%d)", hipGetErrorString(e.code), e.file, e.line);
        rc = (int)e.code;
    }
    if (rc) {  // (buffers a failed init_* allocated before the failing call are not tracked: they stay allocated until the process ends)
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

int grid_close(grid_handle *h) {
    if (!h) return 0;
    GRID_ON_DEVICE(h);
    GRID_GUARDED(
        if (h->f64.hd_data) {  // close_grid frees the streams too: give the f64 state its own (empty) set
            hipStream_t *none = grid::init_grid<double>();
            grid::close_grid<double>(none, h->f64.d_robotModel, h->f64.hd_data);
        }
        grid::close_grid<float>(h->streams, h->f32.d_robotModel, h->f32.hd_data);
        if (h->so_done) (void)hipEventDestroy(h->so_done);
        ee_release(h->ee32);
        ee_release(h->ee64);
    )
    delete h;
    return 0;
}

int grid_device(const grid_handle *h) { return h ? h->device : -1; }

int grid_set_host_chunks(grid_handle *h, int chunks) {
    if (!h || chunks < 0 || chunks > 64) return fail_msg(hipErrorInvalidValue, "grid_set_host_chunks: chunks must be 0 (automatic) .. 64");
    h->host_chunks = chunks;
    return 0;
}
int grid_host_alloc(size_t bytes, void **out) {
    if (!out) return fail_msg(hipErrorInvalidValue, "grid_host_alloc: null result pointer");
    *out = nullptr;
    GRID_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return 0;
}
int grid_host_free(void *p) {
    if (p) GRID_TRY(hipHostFree(p));
    return 0;
}

int grid_set_launch_dims(grid_handle *h, int blocks, int threads) {
    if (!h) return (int)hipErrorInvalidValue;
    if (blocks < 0 || (threads != 0 && (threads < grid::GRID_MIN_THREADS || threads > grid::GRID_MAX_THREADS))) {
        snprintf(g_err, sizeof(g_err), "threads per block must be 0 or in [%d, %d] (whole lane groups; robots with 8-lane groups: whole 16-lane rows), blocks >= 0", grid::GRID_MIN_THREADS, grid::GRID_MAX_THREADS);
        return (int)hipErrorInvalidConfiguration;
    }
    h->blocks = blocks;
    h->threads = threads;
    return 0;
}

// ---- float
int grid_forward_dynamics_gradient_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, int num_timesteps, float gravity, float *d_df_du, void *stream) {
    GRID_GUARDED(return fd_grad_device<float>(h, d_q_qd_u, stride_q_qd_u, num_timesteps, gravity, d_df_du, stream);)
}
int grid_forward_dynamics_gradient_qdd_minv_device(grid_handle *h, const float *d_q_qd, int stride_q_qd, const float *d_qdd, const float *d_Minv,
                                                   int num_timesteps, float gravity, float *d_df_du, void *stream) {
    GRID_GUARDED(return fd_grad_qdd_minv_device<float>(h, d_q_qd, stride_q_qd, d_qdd, d_Minv, num_timesteps, gravity, d_df_du, stream);)
}
int grid_inverse_dynamics_device(grid_handle *h, const float *d_q_qd, int stride_q_qd, const float *d_qdd, int num_timesteps, float gravity, float *d_c, void *stream) {
    GRID_GUARDED(return id_device<float>(h, d_q_qd, stride_q_qd, d_qdd, num_timesteps, gravity, d_c, stream);)
}
int grid_inverse_dynamics_gradient_device(grid_handle *h, const float *d_q_qd, int stride_q_qd, const float *d_qdd, int num_timesteps, float gravity,
                                          float *d_dc_du, void *stream) {
    GRID_GUARDED(return id_grad_device<float>(h, d_q_qd, stride_q_qd, d_qdd, num_timesteps, gravity, d_dc_du, stream);)
}
int grid_direct_minv_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_Minv, void *stream) {
    GRID_GUARDED(return minv_device<float>(h, d_q, stride_q, num_timesteps, d_Minv, stream);)
}
int grid_forward_dynamics_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, int num_timesteps, float gravity, float *d_qdd, void *stream) {
    GRID_GUARDED(return fd_device<float>(h, d_q_qd_u, stride_q_qd_u, num_timesteps, gravity, d_qdd, stream, false);)
}
int grid_aba_device(grid_handle *h, const float *d_q_qd_tau, int stride_q_qd, int num_timesteps, float gravity, float *d_qdd, void *stream) {
    GRID_GUARDED(return fd_device<float>(h, d_q_qd_tau, stride_q_qd, num_timesteps, gravity, d_qdd, stream, true);)
}
int grid_idsva_so_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, const float *d_qdd, int num_timesteps, float gravity, float *d_idsva_so, void *stream) {
    GRID_GUARDED(return idsva_so_device<float>(h, d_q_qd_u, stride_q_qd_u, d_qdd, num_timesteps, gravity, d_idsva_so, stream);)
}
int grid_fdsva_so_device(grid_handle *h, const float *d_q_qd_u, int stride_q_qd_u, int num_timesteps, float gravity, float *d_df2, void *stream) {
    GRID_GUARDED(return fdsva_so_device<float>(h, d_q_qd_u, stride_q_qd_u, num_timesteps, gravity, d_df2, stream);)
}

int grid_forward_dynamics_gradient_host(grid_handle *h, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_df_du) {
    GRID_GUARDED(return fd_grad_host<float>(h, h_q_qd_u, num_timesteps, gravity, h_df_du);)
}
int grid_forward_dynamics_gradient_qdd_minv_host(grid_handle *h, const float *h_q_qd, int stride_q_qd, const float *h_qdd, const float *h_Minv, int num_timesteps,
                                                 float gravity, float *h_df_du) {
    GRID_GUARDED(return fd_grad_qdd_minv_host<float>(h, h_q_qd, stride_q_qd, h_qdd, h_Minv, num_timesteps, gravity, h_df_du);)
}
int grid_inverse_dynamics_host(grid_handle *h, const float *h_q_qd, int stride_q_qd, const float *h_qdd, int num_timesteps, float gravity, float *h_c) {
    GRID_GUARDED(return id_host<float>(h, h_q_qd, stride_q_qd, h_qdd, num_timesteps, gravity, h_c, 0);)
}
int grid_inverse_dynamics_gradient_host(grid_handle *h, const float *h_q_qd, int stride_q_qd, const float *h_qdd, int num_timesteps, float gravity, float *h_dc_du) {
    GRID_GUARDED(return id_host<float>(h, h_q_qd, stride_q_qd, h_qdd, num_timesteps, gravity, h_dc_du, 1);)
}
int grid_direct_minv_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_Minv) {
    GRID_GUARDED(return minv_host<float>(h, h_q, stride_q, num_timesteps, h_Minv);)
}
int grid_forward_dynamics_host(grid_handle *h, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_qdd) {
    GRID_GUARDED(return fd_host<float>(h, h_q_qd_u, num_timesteps, gravity, h_qdd, false);)
}
int grid_aba_host(grid_handle *h, const float *h_q_qd_tau, int num_timesteps, float gravity, float *h_qdd) {
    GRID_GUARDED(return fd_host<float>(h, h_q_qd_tau, num_timesteps, gravity, h_qdd, true);)
}
int grid_idsva_so_host(grid_handle *h, const float *h_q_qd_u, const float *h_qdd, int num_timesteps, float gravity, float *h_idsva_so) {
    GRID_GUARDED(return so_host<float>(h, h_q_qd_u, h_qdd, num_timesteps, gravity, h_idsva_so, 0);)
}
int grid_fdsva_so_host(grid_handle *h, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_df2) {
    GRID_GUARDED(return so_host<float>(h, h_q_qd_u, nullptr, num_timesteps, gravity, h_df2, 1);)
}
int grid_forward_dynamics_gradient_multi_host(grid_handle **handles, int num_handles, const float *h_q_qd_u, int num_timesteps, float gravity, float *h_df_du) {
    GRID_GUARDED(return fd_grad_multi_host<float>(handles, num_handles, h_q_qd_u, num_timesteps, gravity, h_df_du);)
}

// ---- double: the T = double instantiations of the same generated kernels (buffers allocated by the first *_f64 call)
int grid_forward_dynamics_gradient_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, int num_timesteps, double gravity, double *d_df_du, void *stream) {
    GRID_GUARDED(return fd_grad_device<double>(h, d_q_qd_u, stride_q_qd_u, num_timesteps, gravity, d_df_du, stream);)
}
int grid_forward_dynamics_gradient_qdd_minv_device_f64(grid_handle *h, const double *d_q_qd, int stride_q_qd, const double *d_qdd, const double *d_Minv,
                                                       int num_timesteps, double gravity, double *d_df_du, void *stream) {
    GRID_GUARDED(return fd_grad_qdd_minv_device<double>(h, d_q_qd, stride_q_qd, d_qdd, d_Minv, num_timesteps, gravity, d_df_du, stream);)
}
int grid_inverse_dynamics_device_f64(grid_handle *h, const double *d_q_qd, int stride_q_qd, const double *d_qdd, int num_timesteps, double gravity, double *d_c, void *stream) {
    GRID_GUARDED(return id_device<double>(h, d_q_qd, stride_q_qd, d_qdd, num_timesteps, gravity, d_c, stream);)
}
int grid_inverse_dynamics_gradient_device_f64(grid_handle *h, const double *d_q_qd, int stride_q_qd, const double *d_qdd, int num_timesteps, double gravity,
                                              double *d_dc_du, void *stream) {
    GRID_GUARDED(return id_grad_device<double>(h, d_q_qd, stride_q_qd, d_qdd, num_timesteps, gravity, d_dc_du, stream);)
}
int grid_direct_minv_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_Minv, void *stream) {
    GRID_GUARDED(return minv_device<double>(h, d_q, stride_q, num_timesteps, d_Minv, stream);)
}
int grid_forward_dynamics_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, int num_timesteps, double gravity, double *d_qdd, void *stream) {
    GRID_GUARDED(return fd_device<double>(h, d_q_qd_u, stride_q_qd_u, num_timesteps, gravity, d_qdd, stream, false);)
}
int grid_aba_device_f64(grid_handle *h, const double *d_q_qd_tau, int stride_q_qd, int num_timesteps, double gravity, double *d_qdd, void *stream) {
    GRID_GUARDED(return fd_device<double>(h, d_q_qd_tau, stride_q_qd, num_timesteps, gravity, d_qdd, stream, true);)
}
int grid_idsva_so_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, const double *d_qdd, int num_timesteps, double gravity, double *d_idsva_so, void *stream) {
    GRID_GUARDED(return idsva_so_device<double>(h, d_q_qd_u, stride_q_qd_u, d_qdd, num_timesteps, gravity, d_idsva_so, stream);)
}
int grid_fdsva_so_device_f64(grid_handle *h, const double *d_q_qd_u, int stride_q_qd_u, int num_timesteps, double gravity, double *d_df2, void *stream) {
    GRID_GUARDED(return fdsva_so_device<double>(h, d_q_qd_u, stride_q_qd_u, num_timesteps, gravity, d_df2, stream);)
}
int grid_forward_dynamics_gradient_host_f64(grid_handle *h, const double *h_q_qd_u, int num_timesteps, double gravity, double *h_df_du) {
    GRID_GUARDED(return fd_grad_host<double>(h, h_q_qd_u, num_timesteps, gravity, h_df_du);)
}
int grid_inverse_dynamics_host_f64(grid_handle *h, const double *h_q_qd, int stride_q_qd, const double *h_qdd, int num_timesteps, double gravity, double *h_c) {
    GRID_GUARDED(return id_host<double>(h, h_q_qd, stride_q_qd, h_qdd, num_timesteps, gravity, h_c, 0);)
}
int grid_inverse_dynamics_gradient_host_f64(grid_handle *h, const double *h_q_qd, int stride_q_qd, const double *h_qdd, int num_timesteps, double gravity, double *h_dc_du) {
    GRID_GUARDED(return id_host<double>(h, h_q_qd, stride_q_qd, h_qdd, num_timesteps, gravity, h_dc_du, 1);)
}
int grid_direct_minv_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_Minv) {
    GRID_GUARDED(return minv_host<double>(h, h_q, stride_q, num_timesteps, h_Minv);)
}
int grid_forward_dynamics_host_f64(grid_handle *h, const double *h_q_qd_u, int num_timesteps, double gravity, double *h_qdd) {
    GRID_GUARDED(return fd_host<double>(h, h_q_qd_u, num_timesteps, gravity, h_qdd, false);)
}
int grid_aba_host_f64(grid_handle *h, const double *h_q_qd_tau, int num_timesteps, double gravity, double *h_qdd) {
    GRID_GUARDED(return fd_host<double>(h, h_q_qd_tau, num_timesteps, gravity, h_qdd, true);)
}
int grid_idsva_so_host_f64(grid_handle *h, const double *h_q_qd_u, const double *h_qdd, int num_timesteps, double gravity, double *h_idsva_so) {
    GRID_GUARDED(return so_host<double>(h, h_q_qd_u, h_qdd, num_timesteps, gravity, h_idsva_so, 0);)
}
int grid_fdsva_so_host_f64(grid_handle *h, const double *h_q_qd_u, int num_timesteps, double gravity, double *h_df2) {
    GRID_GUARDED(return so_host<double>(h, h_q_qd_u, nullptr, num_timesteps, gravity, h_df2, 1);)
}

// ---- end-effector kinematics
int grid_num_end_effectors(void) { return grid::NUM_EES; }
int grid_end_effector_joints(int *out) {
    if (!out) return fail_msg(hipErrorInvalidValue, "grid_end_effector_joints: null result pointer");
    for (int e = 0; e < grid::NUM_EES; e++) out[e] = grid::GRID_EE_JOINTS[e];
    return 0;
}
int grid_end_effector_pose_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_eePos, void *stream) {
    GRID_GUARDED(return ee_device<float>(h, d_q, stride_q, num_timesteps, d_eePos, nullptr, stream, 0);)
}
int grid_end_effector_pose_gradient_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_deePos, void *stream) {
    GRID_GUARDED(return ee_device<float>(h, d_q, stride_q, num_timesteps, d_deePos, nullptr, stream, 1);)
}
int grid_end_effector_pose_gradient_hessian_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_d2eePos, float *d_deePos, void *stream) {
    GRID_GUARDED(return ee_device<float>(h, d_q, stride_q, num_timesteps, d_d2eePos, d_deePos, stream, 2);)
}
int grid_end_effector_pose_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_eePos) {
    GRID_GUARDED(return ee_host<float>(h, h_q, stride_q, num_timesteps, h_eePos, nullptr, 0);)
}
int grid_end_effector_pose_gradient_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_deePos) {
    GRID_GUARDED(return ee_host<float>(h, h_q, stride_q, num_timesteps, h_deePos, nullptr, 1);)
}
int grid_end_effector_pose_gradient_hessian_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_d2eePos, float *h_deePos) {
    GRID_GUARDED(return ee_host<float>(h, h_q, stride_q, num_timesteps, h_d2eePos, h_deePos, 2);)
}
int grid_end_effector_pose_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_eePos, void *stream) {
    GRID_GUARDED(return ee_device<double>(h, d_q, stride_q, num_timesteps, d_eePos, nullptr, stream, 0);)
}
int grid_end_effector_pose_gradient_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_deePos, void *stream) {
    GRID_GUARDED(return ee_device<double>(h, d_q, stride_q, num_timesteps, d_deePos, nullptr, stream, 1);)
}
int grid_end_effector_pose_gradient_hessian_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_d2eePos, double *d_deePos, void *stream) {
    GRID_GUARDED(return ee_device<double>(h, d_q, stride_q, num_timesteps, d_d2eePos, d_deePos, stream, 2);)
}
int grid_end_effector_pose_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_eePos) {
    GRID_GUARDED(return ee_host<double>(h, h_q, stride_q, num_timesteps, h_eePos, nullptr, 0);)
}
int grid_end_effector_pose_gradient_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_deePos) {
    GRID_GUARDED(return ee_host<double>(h, h_q, stride_q, num_timesteps, h_deePos, nullptr, 1);)
}
int grid_end_effector_pose_gradient_hessian_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_d2eePos, double *h_deePos) {
    GRID_GUARDED(return ee_host<double>(h, h_q, stride_q, num_timesteps, h_d2eePos, h_deePos, 2);)
}

int grid_crba_device(grid_handle *h, const float *d_q, int stride_q, int num_timesteps, float *d_M, void *stream) {
    GRID_GUARDED(return crba_device<float>(h, d_q, stride_q, num_timesteps, d_M, stream);)
}
int grid_crba_host(grid_handle *h, const float *h_q, int stride_q, int num_timesteps, float *h_M) {
    GRID_GUARDED(return crba_host<float>(h, h_q, stride_q, num_timesteps, h_M);)
}
int grid_crba_device_f64(grid_handle *h, const double *d_q, int stride_q, int num_timesteps, double *d_M, void *stream) {
    GRID_GUARDED(return crba_device<double>(h, d_q, stride_q, num_timesteps, d_M, stream);)
}
int grid_crba_host_f64(grid_handle *h, const double *h_q, int stride_q, int num_timesteps, double *h_M) {
    GRID_GUARDED(return crba_host<double>(h, h_q, stride_q, num_timesteps, h_M);)
}
int grid_rollout_device(grid_handle *h, const float *d_x0, int stride_x0, const float *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                        float dt, float gravity, float *d_traj, float *d_xT, void *stream) {
    GRID_GUARDED(return rollout_device<float>(h, d_x0, stride_x0, d_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, d_traj, d_xT, stream);)
}
int grid_rollout_host(grid_handle *h, const float *h_x0, int stride_x0, const float *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                      float dt, float gravity, float *h_traj, float *h_xT) {
    GRID_GUARDED(return rollout_host<float>(h, h_x0, stride_x0, h_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, h_traj, h_xT);)
}
int grid_rollout_device_f64(grid_handle *h, const double *d_x0, int stride_x0, const double *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                            double dt, double gravity, double *d_traj, double *d_xT, void *stream) {
    GRID_GUARDED(return rollout_device<double>(h, d_x0, stride_x0, d_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, d_traj, d_xT, stream);)
}
int grid_rollout_host_f64(grid_handle *h, const double *h_x0, int stride_x0, const double *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                          double dt, double gravity, double *h_traj, double *h_xT) {
    GRID_GUARDED(return rollout_host<double>(h, h_x0, stride_x0, h_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, h_traj, h_xT);)
}
int grid_rollout_linearized_device(grid_handle *h, const float *d_x0, int stride_x0, const float *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                                   float dt, float gravity, float *d_traj, float *d_xT, float *d_fx, float *d_fu, void *stream) {
    GRID_GUARDED(return rollout_linearized_device<float>(h, d_x0, stride_x0, d_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, d_traj, d_xT, d_fx, d_fu, stream);)
}
int grid_rollout_linearized_host(grid_handle *h, const float *h_x0, int stride_x0, const float *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps,
                                 float dt, float gravity, float *h_traj, float *h_xT, float *h_fx, float *h_fu) {
    GRID_GUARDED(return rollout_linearized_host<float>(h, h_x0, stride_x0, h_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, h_traj, h_xT, h_fx, h_fu);)
}
int grid_rollout_linearized_device_f64(grid_handle *h, const double *d_x0, int stride_x0, const double *d_u, long stride_u_step, int stride_u_solve, int num_solves,
                                       int num_steps, double dt, double gravity, double *d_traj, double *d_xT, double *d_fx, double *d_fu, void *stream) {
    GRID_GUARDED(return rollout_linearized_device<double>(h, d_x0, stride_x0, d_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, d_traj, d_xT, d_fx, d_fu, stream);)
}
int grid_rollout_linearized_host_f64(grid_handle *h, const double *h_x0, int stride_x0, const double *h_u, long stride_u_step, int stride_u_solve, int num_solves,
                                     int num_steps, double dt, double gravity, double *h_traj, double *h_xT, double *h_fx, double *h_fu) {
    GRID_GUARDED(return rollout_linearized_host<double>(h, h_x0, stride_x0, h_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, h_traj, h_xT, h_fx, h_fu);)
}
#define GRID_FB_ARGS(T, p)                                                                                                                                         \
    grid_handle *h, const T *p##_x0, int stride_x0, const T *p##_u_ff, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, T dt, T gravity,       \
        const T *p##_K, long stride_K_step, long stride_K_solve, const T *p##_x_ref, long stride_xref_step, long stride_xref_solve, const T *p##_u_min,                \
        const T *p##_u_max, T *p##_traj, T *p##_xT, T *p##_u_out
#define GRID_FB_PASS(p)                                                                                                                                          \
    h, p##_x0, stride_x0, p##_u_ff, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, p##_K, stride_K_step, stride_K_solve, p##_x_ref, stride_xref_step, \
        stride_xref_solve, p##_u_min, p##_u_max, p##_traj, p##_xT, p##_u_out
int grid_rollout_feedback_device(GRID_FB_ARGS(float, d), void *stream) { GRID_GUARDED(return rollout_feedback_device<float>(GRID_FB_PASS(d), stream);) }
int grid_rollout_feedback_host(GRID_FB_ARGS(float, h)) { GRID_GUARDED(return rollout_feedback_host<float>(GRID_FB_PASS(h));) }
int grid_rollout_feedback_device_f64(GRID_FB_ARGS(double, d), void *stream) { GRID_GUARDED(return rollout_feedback_device<double>(GRID_FB_PASS(d), stream);) }
int grid_rollout_feedback_host_f64(GRID_FB_ARGS(double, h)) { GRID_GUARDED(return rollout_feedback_host<double>(GRID_FB_PASS(h));) }
#undef GRID_FB_ARGS
#undef GRID_FB_PASS

int grid_rollout_adjoint_device(grid_handle *h, const float *d_traj, const float *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, float dt, float gravity,
                                const float *d_gx, const float *d_gxT, float *d_grad_x0, float *d_grad_u, void *stream) {
    GRID_GUARDED(return rollout_adjoint_device<float>(h, d_traj, d_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, d_gx, d_gxT, d_grad_x0, d_grad_u, stream);)
}
int grid_rollout_adjoint_host(grid_handle *h, const float *h_traj, const float *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, float dt, float gravity,
                              const float *h_gx, const float *h_gxT, float *h_grad_x0, float *h_grad_u) {
    GRID_GUARDED(return rollout_adjoint_host<float>(h, h_traj, h_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, h_gx, h_gxT, h_grad_x0, h_grad_u);)
}
int grid_rollout_adjoint_device_f64(grid_handle *h, const double *d_traj, const double *d_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, double dt,
                                    double gravity, const double *d_gx, const double *d_gxT, double *d_grad_x0, double *d_grad_u, void *stream) {
    GRID_GUARDED(return rollout_adjoint_device<double>(h, d_traj, d_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, d_gx, d_gxT, d_grad_x0, d_grad_u, stream);)
}
int grid_rollout_adjoint_host_f64(grid_handle *h, const double *h_traj, const double *h_u, long stride_u_step, int stride_u_solve, int num_solves, int num_steps, double dt,
                                  double gravity, const double *h_gx, const double *h_gxT, double *h_grad_x0, double *h_grad_u) {
    GRID_GUARDED(return rollout_adjoint_host<double>(h, h_traj, h_u, stride_u_step, stride_u_solve, num_solves, num_steps, dt, gravity, h_gx, h_gxT, h_grad_x0, h_grad_u);)
}

int grid_forward_dynamics_gradient_single_timing(grid_handle *h, const float *h_q_qd_u, int reps, float gravity, float *h_df_du, double *us_per_call) {
    int rc = check_args(h, reps);
    if (rc) return rc;
    const int n = grid::NUM_JOINTS;
    GRID_ON_DEVICE(h);
    GRID_TRY(hipMemcpy(h->f32.hd_data->d_q_qd_u, h_q_qd_u, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice));
    GRID_TRY(hipDeviceSynchronize());
    struct timespec start, end;
    clock_gettime(CLOCK_MONOTONIC, &start);
    hipLaunchKernelGGL((grid::forward_dynamics_gradient_kernel_single_timing<float>), dim3(1), dim3(grid::GRID_LANES_PER_SOLVE < 64 ? 64 : grid::GRID_LANES_PER_SOLVE),
                       (size_t)(64 / grid::GRID_LANES_PER_SOLVE > 0 ? 64 / grid::GRID_LANES_PER_SOLVE : 1) * (grid::GRID_LDS_PER_SOLVE + grid::GRID_OUT_PER_SOLVE) * sizeof(float),
                       0, h->f32.hd_data->d_df_du, h->f32.hd_data->d_q_qd_u, 3 * n, h->f32.d_robotModel, gravity, reps);
    GRID_TRY(hipGetLastError());
    GRID_TRY(hipDeviceSynchronize());
    clock_gettime(CLOCK_MONOTONIC, &end);
    GRID_TRY(hipMemcpy(h_df_du, h->f32.hd_data->d_df_du, (size_t)2 * n * n * sizeof(float), hipMemcpyDeviceToHost));
    if (us_per_call) *us_per_call = time_delta_us_timespec(start, end) / (double)(reps > 0 ? reps : 1);
    return 0;
}

}  // extern "C"
