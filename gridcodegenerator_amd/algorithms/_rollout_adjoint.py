"""Rollout adjoint: gradient of a scalar cost of a trajectory with respect to x0 and every u_t, one launch in reverse time, emitter for the HIP/CDNA4 backend.

What every gradient-based user of a rollout needs (shooting with first-order optimisers, system identification or policy learning through the simulator, the
gradient half of an iLQR line search).  Built from rollout_linearized that is 3n^2 values per solve and step out to HBM and back for ONE product with a
2n-vector.  Here the reverse pass re-linearises every step in LDS with the inner rollout_linearized_device runs and contracts the record with the adjoint
vector on the spot: per step and solve 5n values come in (x_t, u_t, g_t) and n go out (grad_u_t).

Semantics, per solve, for the cost L = sum_t l_t(x_t), x = [q; qd], with g_t = d l_t / d x_t supplied by the caller and A_t, B_t of rollout_linearized:
    lam_T = g_T;   t = T-1 .. 0:  grad_u_t = B_t^T lam_{t+1},  lam_t = g_t + A_t^T lam_{t+1};   grad_x0 = lam_0
With lam = [lq; lv], [Fq | Fv] = fx_t and M^-1 = fu_t one step collapses to three mat-vecs with ONE n-vector:
    w = lv + dt lq;   grad_u_t = dt M^-1 w;   lq' = gq_t + lq + dt Fq^T w;   lv' = gv_t + w + dt Fv^T w
fx is stored [col*n + row]: Fq^T w and Fv^T w are, per column, a dot product of n contiguous LDS values with w; lane c takes columns c and n + c.

Layouts (time-major): traj (T+1, N, 2n) as rollout wrote it; u as rollout; gx (T+1, N, 2n) or nullptr; gxT (N, 2n) or nullptr (added at step T);
grad_x0 (N, 2n) or nullptr; grad_u (T, N, n) or nullptr - always per solve, also for a shared control sequence (the caller sums over the solves).

LDS: the slice of rollout_linearized with lam (2n) and w (n) behind it; staging: the image of rollout_linearized (fx is assembled in it and consumed in place,
grad_u_t and grad_x0 pass through the head of the wave's first image).  The linearisation is rollout_linearize_device: the inner calls of
rollout_linearized_device without its state update (that function keeps its text; the adjoint does not call it).
"""
from ._rollout_common import _pad4, gen_rollout_family_host, gen_rollout_family_reserve, gen_rollout_kernel_head, gen_rollout_save, gen_rollout_step_loop


def gen_rollout_adjoint_layout(self):
    """(elements of the slice, offset of lam, block size)"""
    n = self.model.n
    total_lin = self.gen_rollout_linearized_layout()[0]
    G = self.lanes_per_solve
    off_lam = _pad4(total_lin)
    total = off_lam + _pad4(3 * n)
    if (total // 4) % 2 == 0:  # (an odd number of 16-byte pieces: the slices of a wave's solves do not start on the same banks)
        total += 4
    out = _pad4(2 * n * n)
    threads = self.suggested_threads
    while threads > 64 and (threads // G) * (total + out) * 4 > 64 * 1024:  # (a block stays inside the default dynamic LDS limit in fp32)
        threads //= 2
    return total, off_lam, max(threads, G)


def gen_rollout_adjoint_constants(self):
    n = self.model.n
    total, off_lam, threads = self.gen_rollout_adjoint_layout()
    self.gen_add_code_line("//")
    self.gen_add_code_line("// rollout_adjoint: T reverse steps of (forward dynamics gradient, M^-1, three mat-vecs with the adjoint vector) in one launch.  Slice: the one of rollout_linearized,")
    self.gen_add_code_line("// lam (2n) | w (n) at ROLLOUT_ADJ_OFF_LAM behind it; staging: ONE image of 2n^2 values per solve (fx, consumed in place; then the grad_u row)")
    self.gen_add_code_line("//")
    self.gen_add_code_lines(["const int ROLLOUT_ADJ_LDS_PER_SOLVE = %d; const int ROLLOUT_ADJ_OUT_PER_SOLVE = %d; const int ROLLOUT_ADJ_SUGGESTED_THREADS = %d; const int ROLLOUT_ADJ_OFF_LAM = %d;"
                             % (total, _pad4(2 * n * n), threads, off_lam),
                             "const int ROLLOUT_ADJ_DYNAMIC_SHARED_MEM_COUNT = (ROLLOUT_ADJ_SUGGESTED_THREADS/GRID_LANES_PER_SOLVE)*(ROLLOUT_ADJ_LDS_PER_SOLVE + ROLLOUT_ADJ_OUT_PER_SOLVE);"])


def gen_rollout_linearize_device(self, use_thread_group=False):
    n = self.model.n
    branch = getattr(self, "branch_frame", False)
    tip_only = self.tip_frame and not branch
    self.gen_add_func_doc("The linearisation of one rollout step in LDS and nothing else: forward dynamics gradient at (q, qd, u), M^-1 from the same pass where the formulation has it "
                          "(lane-group cooperative; the inner calls of rollout_linearized_device without its state update)",
                          ["all lanes of the solve's lane group must call it; on return s_fx holds [d qdd/dq | d qdd/dqd], &s_work[ROLLOUT_LIN_OFF_MINV] the dense M^-1",
                           "(leading dimension GRID_MINV_LD, the triangle row <= col at [col*GRID_MINV_LD + row] is the valid one; only with want_fu); s_q, s_qd, s_tau are left as they were"],
                          ["s_fx is a pointer to LDS for the gradient record of size 2*NUM_JOINTS*NUM_JOINTS = " + str(2 * n * n),
                           "s_q is the vector of joint positions in LDS", "s_qd is the vector of joint velocities in LDS", "s_tau is the vector of joint torques in LDS",
                           "s_work is this solve's LDS workspace of ROLLOUT_LIN_LDS_PER_SOLVE elements",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU", "gravity is the gravity constant",
                           "lane is the caller's lane index inside the solve's lane group",
                           "want_fu (uniform over the lane group): false skips the work that only M^-1 needs"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void rollout_linearize_device(T *s_fx, const T *s_q, const T *s_qd, const T *s_tau, T *s_work, const robotModel<T> *d_robotModel, const T gravity, const int lane, const bool want_fu = true) {", True)
    self.gen_add_code_line("T *s_qdd = &s_work[ROLLOUT_LIN_OFF_QDD]; T *s_Minv = &s_work[ROLLOUT_LIN_OFF_MINV];")
    if tip_only:
        self.gen_add_code_line("// (tip-frame inner: M^-1 comes from the register factors of the gradient pass, one more unit-vector solve per lane)")
        self.gen_add_code_line("forward_dynamics_gradient_device<T>(s_fx, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane, s_qdd, want_fu ? s_Minv : static_cast<T *>(nullptr));")
    elif branch:
        self.gen_add_code_line("// (branch-frame inner: the factors stay parked, so M^-1 is a second call - into direct_minv - and only on demand)")
        self.gen_add_code_line("forward_dynamics_gradient_device<T>(s_fx, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane); (void)s_qdd;")
        self.gen_add_code_line("if (want_fu) { const int lane_m = grid_loop_variant(lane); direct_minv_device<T>(s_Minv, s_q, s_work, d_robotModel, lane_m, ROLLOUT_LIN_OFF_SP); } // (opaque lane: no per-lane constant of the gradient stays in registers for this call)")
    else:
        self.gen_add_code_line("// (column walk: forward_dynamics_inner has left the dense M^-1 in the general slice, the gradient walk reads it and does not overwrite it)")
        self.gen_add_code_line("forward_dynamics_gradient_device<T>(s_fx, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane); (void)want_fu; (void)s_Minv; (void)s_qdd;")
    self.gen_add_end_function()


def gen_rollout_adjoint_prefetch(self):
    """True where the kernel requests g_t and the row of step t-1 BEFORE the dynamics of step t (five registers live across it).  tuning['adjoint_prefetch'] = auto: every
    robot whose lane groups are narrower than 32 lanes; the gradient inner of wider robots (more than 16 joints) sits at the register ceiling, the five values would
    go to scratch there, and such a robot loads them after the dynamics instead."""
    want = self.tuning["adjoint_prefetch"]
    return self.lanes_per_solve < 32 if want == "auto" else bool(want)


def gen_rollout_adjoint_device(self, use_thread_group=False):
    n = self.model.n
    ld = self.minv_ld
    self.gen_add_func_doc("The contraction of one reverse step of the rollout adjoint in LDS: lam_t = g_t + A_t^T lam_{t+1} and grad_u_t = B_t^T lam_{t+1} as three mat-vecs with "
                          "w = lv + dt*lq, from the records rollout_linearize_device left (lane-group cooperative)",
                          ["all lanes of the solve's lane group must call it; on entry s_lam holds lam_{t+1} = [lq | lv], on return lam_t, and s_gu holds grad_u_t (only with want_gu)",
                           "s_gu may alias s_fx: it is written after every lane of the wave has finished reading s_fx",
                           "gq, gv are this lane's entries of g_t = d l_t / d x_t (joint `lane` of the q and of the qd half)"],
                          ["s_gu receives grad_u_t (NUM_JOINTS values in LDS)", "s_lam is the adjoint vector in LDS (2*NUM_JOINTS, updated)", "s_w is LDS scratch of NUM_JOINTS values",
                           "s_fx is the gradient record [d qdd/dq | d qdd/dqd] of step t in LDS, fx[col*n + row]",
                           "s_Minv is the dense M^-1 of step t in LDS (leading dimension GRID_MINV_LD, the triangle row <= col at [col*GRID_MINV_LD + row] is read; only with want_gu)",
                           "dt is the time step", "lane is the caller's lane index inside the solve's lane group", "gq is d l_t / d q_t[lane]", "gv is d l_t / d qd_t[lane]",
                           "want_gu (uniform over the lane group): false skips grad_u_t"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void rollout_adjoint_contract_device(T *s_gu, T *s_lam, T *s_w, const T *s_fx, const T *s_Minv, const T dt, const int lane, const T gq, const T gv, const bool want_gu = true) {", True)
    self.gen_add_code_line("grid_wave_sync();")
    self.gen_add_code_line("if (lane < %d) { s_w[lane] = s_lam[%d + lane] + dt*s_lam[lane]; }" % (n, n))
    self.gen_add_code_line("grid_wave_sync();")
    self.gen_add_code_line("T a_q = static_cast<T>(0), a_v = static_cast<T>(0), a_u = static_cast<T>(0);")
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_line("const T *s_Fq = &s_fx[lane*%d]; const T *s_Fv = &s_fx[(%d + lane)*%d]; // columns lane and n + lane of fx: n contiguous values each" % (n, n, n))
    self.gen_add_code_line("#pragma unroll")
    self.gen_add_code_line("for (int r = 0; r < %d; r++) { const T w = s_w[r]; a_q += s_Fq[r]*w; a_v += s_Fv[r]*w; }" % n)
    self.gen_add_code_line("if (want_gu) { // row `lane` of the symmetric M^-1, read from its valid triangle (as the fu gather of rollout_linearized_kernel)", True)
    self.gen_add_code_line("#pragma unroll")
    self.gen_add_code_line("for (int r = 0; r < %d; r++) { a_u += ((r <= lane) ? s_Minv[lane*%d + r] : s_Minv[r*%d + lane])*s_w[r]; }" % (n, ld, ld))
    self.gen_add_end_control_flow()
    self.gen_add_code_line("a_q = gq + s_lam[lane] + dt*a_q; a_v = gv + s_w[lane] + dt*a_v; a_u = dt*a_u;")
    self.gen_add_end_control_flow()
    self.gen_add_code_line("grid_wave_sync(); // (every lane of the wave is done with s_fx, s_w and s_lam: s_gu may lie inside another solve's image)")
    self.gen_add_code_line("if (lane < %d) { s_lam[lane] = a_q; s_lam[%d + lane] = a_v; if (want_gu) { s_gu[lane] = a_u; } }" % (n, n))
    self.gen_add_sync(use_thread_group)
    self.gen_add_end_function()

    self.gen_add_func_doc("One reverse step of the rollout adjoint in LDS: rollout_linearize_device at (x_t, u_t), then rollout_adjoint_contract_device (lane-group cooperative)",
                          ["all lanes of the solve's lane group must call it; on entry s_lam holds lam_{t+1} = [lq | lv], on return lam_t, and s_gu holds grad_u_t (only with want_gu)",
                           "s_gu may alias s_fx; gq, gv are this lane's entries of g_t = d l_t / d x_t"],
                          ["s_gu receives grad_u_t (NUM_JOINTS values in LDS)", "s_lam is the adjoint vector in LDS (2*NUM_JOINTS, updated)", "s_w is LDS scratch of NUM_JOINTS values",
                           "s_fx is a pointer to LDS for the gradient record of size 2*NUM_JOINTS*NUM_JOINTS = " + str(2 * n * n),
                           "s_q is the vector of joint positions of step t in LDS", "s_qd is the vector of joint velocities of step t in LDS",
                           "s_tau is the vector of joint torques of step t in LDS",
                           "s_work is this solve's LDS workspace of ROLLOUT_LIN_LDS_PER_SOLVE elements",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU", "dt is the time step", "gravity is the gravity constant",
                           "lane is the caller's lane index inside the solve's lane group", "gq is d l_t / d q_t[lane]", "gv is d l_t / d qd_t[lane]",
                           "want_gu (uniform over the lane group): false skips M^-1 and grad_u_t"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void rollout_adjoint_device(T *s_gu, T *s_lam, T *s_w, T *s_fx, const T *s_q, const T *s_qd, const T *s_tau, T *s_work, const robotModel<T> *d_robotModel, "
                           "const T dt, const T gravity, const int lane, const T gq, const T gv, const bool want_gu = true) {", True)
    self.gen_add_code_line("rollout_linearize_device<T>(s_fx, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane, want_gu);")
    self.gen_add_code_line("rollout_adjoint_contract_device<T>(s_gu, s_lam, s_w, s_fx, &s_work[ROLLOUT_LIN_OFF_MINV], dt, lane, gq, gv, want_gu);")
    self.gen_add_end_function()


def gen_rollout_adjoint_kernel(self, use_thread_group=False, single_call_timing=False):
    n = self.model.n
    func_params = ["d_grad_x0 is (NUM_TIMESTEPS, 2n): d cost / d x0 = lam_0, or nullptr",
                   "d_grad_u is (NUM_STEPS, NUM_TIMESTEPS, n): d cost / d u_t of every solve (also when the control is shared: sum over the solves then), or nullptr (the work only M^-1 needs is then skipped)",
                   "d_traj is the state trajectory (NUM_STEPS+1, NUM_TIMESTEPS, 2n) that rollout / rollout_linearized wrote for d_u (row NUM_STEPS is not read)",
                   "d_u is the control: element (t, k, j) at d_u[t*stride_u_step + k*stride_u_solve + j]",
                   "stride_u_step is the stride between the steps of d_u",
                   "stride_u_solve is the stride between the solves of d_u (0: every solve follows the same sequence)",
                   "d_gx is (NUM_STEPS+1, NUM_TIMESTEPS, 2n): d cost / d traj, or nullptr",
                   "d_gxT is (NUM_TIMESTEPS, 2n): d cost / d x_T, added to row NUM_STEPS of d_gx, or nullptr",
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU (XImats, topology_helpers, etc.)",
                   "dt is the time step", "gravity is the gravity constant",
                   "NUM_TIMESTEPS is the number of independent solves (trajectories)",
                   "NUM_STEPS is the number of steps every solve took"]
    func_def = "void rollout_adjoint_kernel(T *d_grad_x0, T *d_grad_u, const T *d_traj, const T *d_u, const long stride_u_step, const int stride_u_solve, const T *d_gx, const T *d_gxT, " \
               "const robotModel<T> *d_robotModel, const T dt, const T gravity, const int NUM_TIMESTEPS, const int NUM_STEPS) {"
    notes = ["lam stays in the solve's LDS slice for all NUM_STEPS steps; the step loop is a runtime loop, in reverse time, around ONE copy of the step",
             ("the row of the step before (x_{t-1}, u_{t-1}) and g_t are loaded into five registers before the dynamics of step t and used after it (no pointer is kept alive across the dynamics)"
              if self.gen_rollout_adjoint_prefetch() else "the row of the step before (x_{t-1}, u_{t-1}) and g_t are loaded after the dynamics of step t (no register is held across it)"),
             "grad_u_t leaves through the head of the wave's first staging image; every row offset is 64-bit",
             "lane groups past the end of the batch walk the loop on the last solve's data and store nothing"]
    if single_call_timing:
        func_def = func_def.replace("kernel(", "kernel_single_timing(")
        notes = ["one solve (record 0) on the first lane group: NUM_TIMESTEPS is ignored, d_traj and d_gx are (NUM_STEPS+1, 2n), d_gxT and d_grad_x0 (2n), d_grad_u (NUM_STEPS, n)"]
    self.gen_add_func_doc("Walk NUM_TIMESTEPS independent trajectories backwards by NUM_STEPS steps and write the gradient of a trajectory cost with respect to x0 and every control", notes, func_params, None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__global__ GRID_LAUNCH_BOUNDS")
    self.gen_add_code_line(func_def, True)
    self.gen_kernel_prologue("ROLLOUT_ADJ_LDS_PER_SOLVE")
    self.gen_add_code_lines(["T *s_x = &s_mem[GRID_OFF_IN]; T *s_q = s_x; T *s_qd = &s_x[%d]; T *s_tau = &s_x[%d]; T *s_lam = &s_mem[ROLLOUT_ADJ_OFF_LAM]; T *s_w = &s_lam[%d];" % (n, 2 * n, 2 * n),
                             "// the staging image of this solve; grad_u_t and grad_x0 go through the head of the image of the wave's first solve (images of other waves are never touched)",
                             "T *s_fx = &s_out_all[grp*%d];" % (2 * n * n),
                             "T *s_gu = &s_out_all[(grp & ~(GRID_SOLVES_PER_WAVE-1))*%d + (grp & (GRID_SOLVES_PER_WAVE-1))*%d];" % (2 * n * n, n),
                             "T *s_out = &s_out_all[(grp & ~(GRID_SOLVES_PER_WAVE-1))*%d + (grp & (GRID_SOLVES_PER_WAVE-1))*%d];" % (2 * n * n, 2 * n)])
    gen_rollout_kernel_head(self, [("row", 2 * n), ("gu", n)], "d_traj / d_gx, d_grad_u", single_call_timing, use_thread_group, valid_unused=True)
    self.gen_add_code_line("// lam_T = g_T (+ gxT) and the row of step T-1: [q | qd] of d_traj, u")
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_line("const size_t xk = static_cast<size_t>(kc)*%d + lane;" % (2 * n))
    self.gen_add_code_line("T lq = static_cast<T>(0), lv = static_cast<T>(0);")
    self.gen_add_code_line("if (d_gx != nullptr) { const T *d_g = d_gx + static_cast<size_t>(NUM_STEPS)*row_stride + xk; lq = d_g[0]; lv = d_g[%d]; }" % n)
    self.gen_add_code_line("if (d_gxT != nullptr) { lq += d_gxT[xk]; lv += d_gxT[xk + %d]; }" % n)
    self.gen_add_code_line("if (NUM_STEPS > 0) {", True)
    self.gen_add_code_line("const T *d_x = d_traj + static_cast<size_t>(NUM_STEPS - 1)*row_stride + xk;")
    self.gen_add_code_line("s_q[lane] = d_x[0]; s_qd[lane] = d_x[%d]; s_tau[lane] = d_u[static_cast<long>(NUM_STEPS - 1)*stride_u_step + static_cast<long>(kc)*stride_u_solve + lane];" % n)
    self.gen_add_end_control_flow()
    self.gen_add_code_line("s_lam[lane] = lq; s_lam[%d + lane] = lv;" % n)
    self.gen_add_end_control_flow()
    self.gen_add_sync(use_thread_group)
    gen_rollout_step_loop(self, reverse=True)
    prefetch = self.gen_rollout_adjoint_prefetch()
    kk = "kc" if single_call_timing else "(k < NUM_TIMESTEPS ? k : NUM_TIMESTEPS - 1)"

    def load_row():
        self.gen_add_code_line("T r_gq = static_cast<T>(0), r_gv = static_cast<T>(0), r_q = static_cast<T>(0), r_qd = static_cast<T>(0), r_u = static_cast<T>(0);")
        self.gen_add_code_line("if (lane < %d) {" % n, True)
        self.gen_add_code_line("const int kk = %s; const int xo = kk*%d + lane; // (one row of d_traj holds fewer than 2^31 values: the C entry points check it)" % (kk, 2 * n))
        self.gen_add_code_line("if (d_gx != nullptr) { const T *d_g = d_gx + static_cast<size_t>(t)*row_stride; r_gq = d_g[xo]; r_gv = d_g[xo + %d]; }" % n)
        self.gen_add_code_line("if (t > 0) {", True)
        self.gen_add_code_line("const T *d_x = d_traj + static_cast<size_t>(t - 1)*row_stride; const T *d_u_t = d_u + static_cast<long>(t - 1)*stride_u_step;")
        self.gen_add_code_line("r_q = d_x[xo]; r_qd = d_x[xo + %d]; r_u = d_u_t[static_cast<long>(kk)*stride_u_solve + lane];" % n)
        self.gen_add_end_control_flow()
        self.gen_add_end_control_flow()

    if prefetch:
        self.gen_add_code_line("// g_t and the row of step t-1 leave for the registers now; g_t is used after the dynamics, the row lands in LDS after this step")
        self.gen_add_code_line("// (wave-uniform 64-bit bases + 32-bit lane offsets, rebuilt from k every step: no pointer is kept alive across the dynamics)")
        load_row()
        self.gen_add_code_line("rollout_adjoint_device<T>(s_gu, s_lam, s_w, s_fx, s_q, s_qd, s_tau, s_mem, d_robotModel, dt, gravity, lane, r_gq, r_gv, d_grad_u != nullptr);")
    else:
        self.gen_add_code_line("rollout_linearize_device<T>(s_fx, s_q, s_qd, s_tau, s_mem, d_robotModel, gravity, lane, d_grad_u != nullptr);")
        self.gen_add_code_line("// g_t and the row of step t-1 are loaded AFTER the dynamics: this robot's gradient inner leaves no five registers free across it (gen_rollout_adjoint_prefetch)")
        load_row()
        self.gen_add_code_line("rollout_adjoint_contract_device<T>(s_gu, s_lam, s_w, s_fx, &s_mem[ROLLOUT_LIN_OFF_MINV], dt, lane, r_gq, r_gv, d_grad_u != nullptr);")
    self.gen_add_code_line("if (d_grad_u != nullptr) {", True)
    gen_rollout_save(self, "d_grad_u + static_cast<size_t>(t)*gu_stride", "gu_t", n, "s_gu", single_call_timing, use_thread_group)
    self.gen_add_end_control_flow()
    self.gen_add_code_line("if (t > 0 && lane < %d) { s_q[lane] = r_q; s_qd[lane] = r_qd; s_tau[lane] = r_u; }" % n)
    self.gen_add_sync(use_thread_group)
    self.gen_add_end_control_flow()
    self.gen_add_code_line("if (d_grad_x0 != nullptr) { // lam_0", True)
    gen_rollout_save(self, "d_grad_x0", "gx0_k", 2 * n, "s_out", single_call_timing, use_thread_group, "s_lam")
    self.gen_add_end_control_flow()
    if not single_call_timing:
        self.gen_add_end_control_flow()
    self.gen_add_end_function()


ROLLOUT_ADJOINT_RESERVE = dict(
    name="rollout_adjoint", base="rollout", min_steps=0,
    doc=("Reserves the buffers of the rollout adjoint for num_timesteps solves of num_steps steps (those of rollout_reserve, the cotangent of the trajectory and the two gradients)",
         ["d_gx_traj / h_gx_traj: (num_steps+1, num_timesteps, 2n); d_gu_traj / h_gu_traj: (num_steps, num_timesteps, n); d_gx0 / h_gx0: (num_timesteps, 2n)",
          "null after init_gridData; the rollout_adjoint host wrappers call this themselves; grows on demand, close_grid frees"]),
    rows=[("gx_traj", "2*NUM_JOINTS", "(S + 1)*N"), ("gu_traj", "NUM_JOINTS", "(S > 0 ? S : 1)*N"), ("gx0", "2*NUM_JOINTS", "N")])

ROLLOUT_ADJOINT_HOST = dict(
    name="rollout_adjoint", tag="ROLLOUT_ADJ", x0=False,
    doc=("Walk num_timesteps trajectories backwards by num_steps steps and return the gradient of a trajectory cost with respect to x0 and every control",
         ["no counterpart in the reference; call rollout_adjoint_reserve first and fill h_x_traj (rollout leaves its result there), h_u_traj and h_gx_traj",
          "_single_timing: solve 0 alone, num_steps steps in one launch, time per step printed"],
         "the trajectory in h_x_traj (num_steps+1, num_timesteps, 2n), u in h_u_traj (num_steps, num_timesteps, n), "
         "d cost / d traj in h_gx_traj (num_steps+1, num_timesteps, 2n); results in h_gx0 (num_timesteps, 2n) and h_gu_traj (num_steps, num_timesteps, n)", "took"),
    args="hd_data->d_gx0,hd_data->d_gu_traj,hd_data->d_x_traj,hd_data->d_u_traj,stride_u_step,stride_u_solve,hd_data->d_gx_traj,static_cast<const T *>(nullptr),"
         "d_robotModel,dt,gravity,num_timesteps,num_steps);",
    h2d=[("x_traj", "2*NUM_JOINTS", "*(num_steps + 1)"), ("gx_traj", "2*NUM_JOINTS", "*(num_steps + 1)"), ("u_traj", "NUM_JOINTS", "*num_steps")],
    d2h=[("gx0", "2*NUM_JOINTS", ""), ("gu_traj", "NUM_JOINTS", "*num_steps")])


def gen_rollout_adjoint_reserve(self):
    gen_rollout_family_reserve(self, ROLLOUT_ADJOINT_RESERVE)


def gen_rollout_adjoint_host(self, mode=0):
    gen_rollout_family_host(self, ROLLOUT_ADJOINT_HOST, mode)


def gen_rollout_adjoint(self, use_thread_group=False):
    self.gen_rollout_adjoint_constants()
    self.gen_rollout_linearize_device(use_thread_group)
    self.gen_rollout_adjoint_device(use_thread_group)
    self.gen_rollout_adjoint_kernel(use_thread_group, True)
    self.gen_rollout_adjoint_kernel(use_thread_group, False)
    self.gen_rollout_adjoint_reserve()
    for mode in (0, 1, 2):
        self.gen_rollout_adjoint_host(mode)
