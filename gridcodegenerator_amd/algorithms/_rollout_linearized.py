"""Linearised fused rollout: the trajectory AND the Jacobians of the dynamics along it, emitter for the HIP/CDNA4 backend.

What a shooting method (iLQR / DDP / MPC) needs per iteration: for every step t the next state and the linearisation of the step map at (x_t, u_t).
Built from the existing entry points that is, per step, one forward_dynamics_gradient launch + one direct_minv launch + one aba launch + update
kernels, the state going out to HBM and back between all of them.  Here one launch keeps q, qd and u of every solve in its LDS slice for all T steps
and runs ONE dynamics pass per step: the gradient's own factorisation of M delivers qdd (and, where the formulation has it, M^-1).

Semantics, per solve k and step t = 0 .. T-1 (gravity, damping and conventions of rollout; no joint limits, no angle wrapping, no contact):
    qdd_t = FD(q_t, qd_t, u_t)                          the one forward_dynamics_gradient_device computes (not aba_device: rounding-level difference to rollout)
    fx_t  = [d qdd/dq | d qdd/dqd] at (q_t, qd_t, u_t)  the df_du record: fx[col*n + row], n x 2n
    fu_t  = d qdd/du = M^-1(q_t)                        dense, exactly symmetric: fu[col*n + row]
    (q_{t+1}, qd_{t+1}) by grid_symplectic_euler_step   (algorithms/_rollout.py: still the only place the update is written)
The discrete Jacobians A_t, B_t of this integrator follow from fx, fu and dt without further dynamics (runtime.discrete_jacobians).

Layouts (time-major, as rollout): x0, u, traj, xT as rollout; fx (T, N, 2n^2); fu (T, N, n^2); all optional outputs, row offsets in size_t.

Which inner runs (one per formulation of forward_dynamics_gradient):
    tip frame (serial revolute chains, forests of them)   forward_dynamics_gradient_device(..., s_qdd_out, s_Minv_out): qdd and M^-1 from the register factors
    column walk (prismatic joints, deep random trees)     forward_dynamics_gradient_device leaves qdd and the dense M^-1 in the general slice
    branch frame (branched revolute robots, long chains)  forward_dynamics_gradient_device leaves qdd (FD_DU_OFF_QDD); its inner parks the factors and never forms
                                                          M^-1, so direct_minv_device runs as a second call inside the step - only when fu is asked for
LDS: tip frame / column walk / long chains use the general slice; branched robots a compact one (the gradient kernel's slice and direct_minv's compact
slice overlaid, M^-1 behind them).  ONE staging image of 2n^2 values per solve: fx is assembled in it and stored, fu is gathered straight from M^-1 by
the solve's own lanes (16-byte pieces, mirrored from one triangle), then the state row passes through the head of the wave's image.
"""
from ._rollout_common import _pad4, gen_rollout_commit_control, gen_rollout_family_host, gen_rollout_family_reserve, gen_rollout_kernel_head, gen_rollout_load_x0, \
    gen_rollout_prefetch_control, gen_rollout_save, gen_rollout_step_loop


def gen_rollout_linearized_layout(self):
    """(elements of the slice, offset of qdd, offset of M^-1, offset of direct_minv's path-axis scratch, block size)"""
    n = self.model.n
    lds = self.gen_lds_layout()
    G = self.lanes_per_solve
    spw = 64 // G
    if getattr(self, "branch_components", False) and lds["KERNELS"]["MINV"]["compact"]:
        K = lds["KERNELS"]["MINV"]
        total = max(lds["FD_TOTAL"], K["LDS"])
        if (total % 64 == 0) if spw <= 2 else ((total // 4) % 2 == 0):
            total += 4
        off_qdd, off_minv, off_sp = lds["FD_QDD"], K["MINV"], K["SP"]
        assert off_minv + n * self.minv_ld <= total
    else:
        total, off_minv, off_sp = lds["TOTAL"], lds["MINV"], lds["SP"]
        off_qdd = lds["FD_QDD"] if getattr(self, "branch_frame", False) else lds["QDD"]
    out = _pad4(2 * n * n)
    threads = self.suggested_threads
    while threads > 64 and (threads // G) * (total + out) * 4 > 64 * 1024:  # (a block stays inside the default dynamic LDS limit in fp32)
        threads //= 2
    return total, off_qdd, off_minv, off_sp, max(threads, G)


def gen_rollout_linearized_constants(self):
    n = self.model.n
    total, off_qdd, off_minv, off_sp, threads = self.gen_rollout_linearized_layout()
    self.gen_add_code_line("//")
    self.gen_add_code_line("// rollout_linearized: T steps of (forward dynamics gradient, M^-1, symplectic Euler) in one launch.  Slice: q | qd | u resident in GRID_OFF_IN, the gradient's workspace,")
    self.gen_add_code_line("// qdd and the dense M^-1 of the step at ROLLOUT_LIN_OFF_QDD / _OFF_MINV; staging: ONE image of 2n^2 values per solve (fx, then the state row)")
    self.gen_add_code_line("//")
    self.gen_add_code_lines(["const int ROLLOUT_LIN_LDS_PER_SOLVE = %d; const int ROLLOUT_LIN_OUT_PER_SOLVE = %d; const int ROLLOUT_LIN_SUGGESTED_THREADS = %d;" % (total, _pad4(2 * n * n), threads),
                             "const int ROLLOUT_LIN_OFF_QDD = %d; const int ROLLOUT_LIN_OFF_MINV = %d; const int ROLLOUT_LIN_OFF_SP = %d;" % (off_qdd, off_minv, off_sp),
                             "const int ROLLOUT_LIN_DYNAMIC_SHARED_MEM_COUNT = (ROLLOUT_LIN_SUGGESTED_THREADS/GRID_LANES_PER_SOLVE)*(ROLLOUT_LIN_LDS_PER_SOLVE + ROLLOUT_LIN_OUT_PER_SOLVE);"])


def gen_rollout_linearized_device(self, use_thread_group=False):
    n = self.model.n
    branch = getattr(self, "branch_frame", False)
    tip_only = self.tip_frame and not branch
    self.gen_add_func_doc("One linearised rollout step in LDS: forward dynamics gradient at (q, qd, u), qdd and M^-1 from the same pass where the formulation has them, "
                          "then the symplectic Euler update of (q, qd) (lane-group cooperative)",
                          ["all lanes of the solve's lane group must call it; on return s_fx holds [d qdd/dq | d qdd/dqd] of the OLD state, &s_work[ROLLOUT_LIN_OFF_QDD] its qdd,",
                           "&s_work[ROLLOUT_LIN_OFF_MINV] the dense M^-1 of the old q (leading dimension GRID_MINV_LD; only with want_fu) and s_q, s_qd the NEW state"],
                          ["s_fx is a pointer to LDS for the gradient record of size 2*NUM_JOINTS*NUM_JOINTS = " + str(2 * n * n),
                           "s_q is the vector of joint positions in LDS (updated)", "s_qd is the vector of joint velocities in LDS (updated)",
                           "s_tau is the vector of joint torques of this step in LDS",
                           "s_work is this solve's LDS workspace of ROLLOUT_LIN_LDS_PER_SOLVE elements",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU", "dt is the time step", "gravity is the gravity constant",
                           "lane is the caller's lane index inside the solve's lane group",
                           "want_fu (uniform over the lane group): false skips the work that only M^-1 needs"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void rollout_linearized_device(T *s_fx, T *s_q, T *s_qd, const T *s_tau, T *s_work, const robotModel<T> *d_robotModel, const T dt, const T gravity, const int lane, const bool want_fu = true) {", True)
    self.gen_add_code_line("T *s_qdd = &s_work[ROLLOUT_LIN_OFF_QDD]; T *s_Minv = &s_work[ROLLOUT_LIN_OFF_MINV];")
    if tip_only:
        self.gen_add_code_line("// (tip-frame inner: qdd and, with one more unit-vector solve per lane, M^-1 come from the register factors of the gradient pass)")
        self.gen_add_code_line("forward_dynamics_gradient_device<T>(s_fx, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane, s_qdd, want_fu ? s_Minv : static_cast<T *>(nullptr));")
    elif branch:
        self.gen_add_code_line("// (branch-frame inner: qdd is left at FD_DU_OFF_QDD = ROLLOUT_LIN_OFF_QDD; the factors stay parked, so M^-1 is a second call - into direct_minv - and only on demand)")
        self.gen_add_code_line("forward_dynamics_gradient_device<T>(s_fx, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane);")
        self.gen_add_code_line("if (want_fu) { const int lane_m = grid_loop_variant(lane); direct_minv_device<T>(s_Minv, s_q, s_work, d_robotModel, lane_m, ROLLOUT_LIN_OFF_SP); } // (opaque lane: no per-lane constant of the gradient stays in registers for this call)")
    else:
        self.gen_add_code_line("// (column walk: forward_dynamics_inner has left qdd and the dense M^-1 in the general slice, the gradient walk reads both and overwrites neither)")
        self.gen_add_code_line("forward_dynamics_gradient_device<T>(s_fx, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane); (void)want_fu; (void)s_Minv;")
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_line("T q = s_q[lane]; T qd = s_qd[lane];")
    self.gen_add_code_line("grid_symplectic_euler_step(q, qd, s_qdd[lane], dt);")
    self.gen_add_code_line("s_qd[lane] = qd; s_q[lane] = q;")
    self.gen_add_end_control_flow()
    self.gen_add_sync(use_thread_group)
    self.gen_add_end_function()


def gen_rollout_linearized_kernel(self, use_thread_group=False, single_call_timing=False):
    n = self.model.n
    ld = self.minv_ld
    func_params = ["d_traj is the state trajectory (NUM_STEPS+1, NUM_TIMESTEPS, 2n), row 0 is x0, or nullptr",
                   "d_xT is the final state (NUM_TIMESTEPS, 2n), or nullptr",
                   "d_fx is (NUM_STEPS, NUM_TIMESTEPS, 2n^2): [d qdd/dq | d qdd/dqd] at (x_t, u_t), fx[col*n + row], or nullptr",
                   "d_fu is (NUM_STEPS, NUM_TIMESTEPS, n^2): d qdd/du = M^-1(q_t), dense and exactly symmetric, or nullptr (the work only M^-1 needs is then skipped)",
                   "d_x0 is the initial state: the first 2n values of every row are [q | qd]",
                   "stride_x0 is the stride between the rows of d_x0 (>= 2n)",
                   "d_u is the control: element (t, k, j) at d_u[t*stride_u_step + k*stride_u_solve + j]",
                   "stride_u_step is the stride between the steps of d_u",
                   "stride_u_solve is the stride between the solves of d_u (0: every solve follows the same sequence)",
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU (XImats, topology_helpers, etc.)",
                   "dt is the time step", "gravity is the gravity constant",
                   "NUM_TIMESTEPS is the number of independent solves (trajectories)",
                   "NUM_STEPS is the number of steps every solve takes"]
    func_def = "void rollout_linearized_kernel(T *d_traj, T *d_xT, T *d_fx, T *d_fu, const T *d_x0, const int stride_x0, const T *d_u, const long stride_u_step, const int stride_u_solve, " \
               "const robotModel<T> *d_robotModel, const T dt, const T gravity, const int NUM_TIMESTEPS, const int NUM_STEPS) {"
    notes = ["q, qd and u stay in the solve's LDS slice for all NUM_STEPS steps; the step loop is a runtime loop around ONE copy of the step",
             "the control of step t+1 is loaded into a register before the dynamics of step t",
             "fx, fu and the state row leave one after the other through ONE staging image; every row offset is 64-bit",
             "lane groups past the end of the batch walk the loop on the last solve's data and store nothing"]
    if single_call_timing:
        func_def = func_def.replace("kernel(", "kernel_single_timing(")
        notes = ["one solve (record 0) on the first lane group: NUM_TIMESTEPS is ignored, d_traj is (NUM_STEPS+1, 2n), d_xT (2n), d_fx (NUM_STEPS, 2n^2), d_fu (NUM_STEPS, n^2)"]
    self.gen_add_func_doc("Roll NUM_TIMESTEPS independent trajectories forward by NUM_STEPS steps and write the Jacobians of the dynamics at every step", notes, func_params, None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__global__ GRID_LAUNCH_BOUNDS")
    self.gen_add_code_line(func_def, True)
    self.gen_kernel_prologue("ROLLOUT_LIN_LDS_PER_SOLVE")
    self.gen_add_code_lines(["T *s_x = &s_mem[GRID_OFF_IN]; T *s_x0 = s_x; T *s_q = s_x; T *s_qd = &s_x[%d]; T *s_tau = &s_x[%d]; const T *s_Minv = &s_mem[ROLLOUT_LIN_OFF_MINV];" % (n, 2 * n),
                             "// the staging image of this solve; the state row goes through the head of the image of the wave's first solve (images of other waves are never touched)",
                             "T *s_fx = &s_out_all[grp*%d];" % (2 * n * n),
                             "T *s_out = &s_out_all[(grp & ~(GRID_SOLVES_PER_WAVE-1))*%d + (grp & (GRID_SOLVES_PER_WAVE-1))*%d];" % (2 * n * n, 2 * n)])
    gen_rollout_kernel_head(self, [("row", 2 * n), ("fx", 2 * n * n), ("fu", n * n)], "d_traj, d_fx, d_fu", single_call_timing, use_thread_group)
    gen_rollout_load_x0(self, use_thread_group)
    save = lambda row_ptr_expr, name, amount, src, copy_from=None: gen_rollout_save(self, row_ptr_expr, name, amount, src, single_call_timing, use_thread_group, copy_from)
    self.gen_add_code_line("if (d_traj != nullptr) { // row 0 is x0", True)
    save("d_traj", "traj_t", 2 * n, "s_out", "s_x")
    self.gen_add_end_control_flow()
    gen_rollout_step_loop(self)
    self.gen_add_code_line("// the next step's control leaves for the registers now and lands in LDS after this step (no pointer is kept alive across the dynamics)")
    gen_rollout_prefetch_control(self, single_call_timing)
    self.gen_add_code_line("rollout_linearized_device<T>(s_fx, s_q, s_qd, s_tau, s_mem, d_robotModel, dt, gravity, lane, d_fu != nullptr);")
    self.gen_add_code_line("if (d_fx != nullptr) {", True)
    save("d_fx + static_cast<size_t>(t)*fx_stride", "fx_t", 2 * n * n, "s_fx")
    self.gen_add_end_control_flow()
    self.gen_add_code_line("if (d_fu != nullptr && valid) { // dense symmetric record gathered from one triangle of M^-1 by the solve's own lanes: no staging copy", True)
    self.gen_add_code_line("T *dst = d_fu + static_cast<size_t>(t)*fu_stride + static_cast<size_t>(%s)*%d;" % ("kc" if single_call_timing else "grid_loop_variant(k)", n * n))
    self.gen_add_code_line("for (int e = 4*lane; e + 3 < %d; e += 4*GRID_LANES_PER_SOLVE) {" % (n * n), True)
    self.gen_add_code_line("T tmp[4];")
    self.gen_add_code_line("#pragma unroll")
    self.gen_add_code_line("for (int r = 0; r < 4; r++) { const int ind = e + r; const int row = ind %% %d; const int col = ind / %d; tmp[r] = (row <= col) ? s_Minv[col*%d + row] : s_Minv[row*%d + col]; }" % (n, n, ld, ld))
    self.gen_add_code_line("grid_store4(dst + e, tmp);")
    self.gen_add_end_control_flow()
    if (n * n) % 4:
        self.gen_add_code_line("{ const int ind = %d + lane; if (lane < %d) { const int row = ind %% %d; const int col = ind / %d; dst[ind] = (row <= col) ? s_Minv[col*%d + row] : s_Minv[row*%d + col]; } }"
                               % (n * n // 4 * 4, (n * n) % 4, n, n, ld, ld))
    self.gen_add_end_control_flow()
    gen_rollout_commit_control(self, use_thread_group)
    self.gen_add_code_line("if (d_traj != nullptr) {", True)
    save("d_traj + static_cast<size_t>(t + 1)*row_stride", "traj_t", 2 * n, "s_out", "s_x")
    self.gen_add_end_control_flow()
    self.gen_add_end_control_flow()
    self.gen_add_code_line("if (d_xT != nullptr) {", True)
    save("d_xT", "xT_k", 2 * n, "s_out", "s_x")
    self.gen_add_end_control_flow()
    if not single_call_timing:
        self.gen_add_end_control_flow()
    self.gen_add_end_function()


ROLLOUT_LINEARIZED_RESERVE = dict(
    name="rollout_linearized", base="rollout", min_steps=1,
    doc=("Reserves the buffers of the linearised rollout for num_timesteps solves of num_steps steps (those of rollout_reserve and the two Jacobian records)",
         ["d_fx_traj / h_fx_traj: (num_steps, num_timesteps, 2n^2); d_fu_traj / h_fu_traj: (num_steps, num_timesteps, n^2)",
          "null after init_gridData; the rollout_linearized host wrappers call this themselves; grows on demand, close_grid frees"]),
    rows=[("fx_traj", "2*NUM_JOINTS*NUM_JOINTS", "S*N"), ("fu_traj", "NUM_JOINTS*NUM_JOINTS", "S*N")])

ROLLOUT_LINEARIZED_HOST = dict(
    name="rollout_linearized", tag="ROLLOUT_LIN", x0=True,
    doc=("Roll num_timesteps trajectories forward by num_steps steps and return the Jacobians of the dynamics at every step",
         ["no counterpart in the reference; call rollout_linearized_reserve first and fill h_u_traj",
          "_single_timing: solve 0 alone, num_steps steps in one launch, time per step printed"],
         "x0 in h_q_qd_u (rows of 3n, [q | qd | unused]), u in h_u_traj (num_steps, num_timesteps, n); "
         "results in h_x_traj (num_steps+1, num_timesteps, 2n), h_fx_traj (num_steps, num_timesteps, 2n^2), h_fu_traj (num_steps, num_timesteps, n^2)", "takes"),
    args="hd_data->d_x_traj,static_cast<T *>(nullptr),hd_data->d_fx_traj,hd_data->d_fu_traj,hd_data->d_q_qd_u,stride_x0,hd_data->d_u_traj,stride_u_step,stride_u_solve,"
         "d_robotModel,dt,gravity,num_timesteps,num_steps);",
    h2d=[("q_qd_u", "stride_x0", ""), ("u_traj", "NUM_JOINTS", "*num_steps")],
    d2h=[("x_traj", "2*NUM_JOINTS", "*(num_steps + 1)"), ("fx_traj", "2*NUM_JOINTS*NUM_JOINTS", "*num_steps"), ("fu_traj", "NUM_JOINTS*NUM_JOINTS", "*num_steps")])


def gen_rollout_linearized_reserve(self):
    gen_rollout_family_reserve(self, ROLLOUT_LINEARIZED_RESERVE)


def gen_rollout_linearized_host(self, mode=0):
    gen_rollout_family_host(self, ROLLOUT_LINEARIZED_HOST, mode)


def gen_rollout_linearized(self, use_thread_group=False):
    self.gen_rollout_linearized_constants()
    self.gen_rollout_linearized_device(use_thread_group)
    self.gen_rollout_linearized_kernel(use_thread_group, True)
    self.gen_rollout_linearized_kernel(use_thread_group, False)
    self.gen_rollout_linearized_reserve()
    for mode in (0, 1, 2):
        self.gen_rollout_linearized_host(mode)
