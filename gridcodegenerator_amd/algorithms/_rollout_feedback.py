"""Closed-loop rollout: the fused rollout with a time-varying linear feedback law and torque limits applied inside the step loop, emitter for the HIP/CDNA4 backend.

What the forward pass of iLQR / DDP (u_t = u_ff_t + K_t (x_t - x_ref_t), u_ff = u_bar + alpha k is the caller's), tracking under a TVLQR or PD controller and a linear
policy evaluated over many initial conditions need: the control of step t depends on the state the rollout has just reached.  Built from the open-loop members that is
one aba launch per step with a mat-vec, a clamp and the integrator update in between; here the law runs on the state in LDS and the dynamics step is rollout_device.

Semantics, per solve k and step t = 0 .. T-1 (dynamics, gravity convention, damping and integrator of rollout; no joint limits, no wrapping, no contact):
    dx  = x_t - x_ref[t, k]                                x = [q ; qd], 2n values
    v   = u_ff[t, k][j] + sum_c K[t, k][c*n + j]*dx[c]     ONE accumulator that starts from u_ff, c ascending 0 .. 2n-1, one multiply and one add per term
    u_t = v                                                without limits
    u_t = v < u_min[j] ? u_min[j] : (v > u_max[j] ? u_max[j] : v)      with limits (a NaN v stays NaN: a diverged solve remains visible)
    rollout_device(q_t, qd_t, u_t)                         ABA + grid_symplectic_euler_step

Layouts (time-major): x0, traj, xT as rollout; u_ff as the u of rollout (d_u, stride_u_step, stride_u_solve); K element (t, k, c*n + j) at
d_K[t*stride_K_step + k*stride_K_solve + c*n + j] (a step stride of 0: one gain for all steps, a solve stride of 0: one gain for all solves); x_ref element (t, k, i) at
d_xref[t*stride_xref_step + k*stride_xref_solve + i] (step stride 0: a set point, solve stride 0: one reference for all solves; a nominal traj passes as it is);
u_min, u_max n values each, both or neither; u_out (T, N, n), the control that was applied.

LDS: the slice of rollout_kernel with dx (2n) behind it; staging: one [q | qd] row per solve, as rollout_kernel; u_out[t] passes through the head of the wave's staging.
K goes from global memory straight into the multiply-adds: with the [c*n + j] record the n joint lanes of a solve read n contiguous values per column.
"""
from ._rollout_common import _pad4, gen_rollout_family_host, gen_rollout_family_reserve, gen_rollout_kernel_head, gen_rollout_load_x0, gen_rollout_prefetch_control, \
    gen_rollout_save, gen_rollout_step_loop


def gen_rollout_feedback_layout(self):
    """(elements of the slice, offset of dx)"""
    n = self.model.n
    off_dx = _pad4(self.gen_lds_layout()["KERNELS"]["ABA"]["LDS"])
    total = off_dx + _pad4(2 * n)
    if (total // 4) % 2 == 0:  # (an odd number of 16-byte pieces: the slices of a wave's solves do not start on the same banks)
        total += 4
    return total, off_dx


def gen_rollout_feedback_constants(self):
    n = self.model.n
    total, off_dx = self.gen_rollout_feedback_layout()
    self.gen_add_code_line("//")
    self.gen_add_code_line("// rollout_feedback: T steps of (linear feedback law, torque limits, aba, symplectic Euler) in one launch.  Slice: the one of rollout, dx = x - x_ref (2n) at")
    self.gen_add_code_line("// ROLLOUT_FB_OFF_DX behind it; staging: one [q | qd] row per solve (the u_out row passes through the head of the wave's staging)")
    self.gen_add_code_line("//")
    self.gen_add_code_lines(["const int ROLLOUT_FB_LDS_PER_SOLVE = %d; const int ROLLOUT_FB_OUT_PER_SOLVE = ROLLOUT_OUT_PER_SOLVE; const int ROLLOUT_FB_OFF_DX = %d; const int ROLLOUT_FB_SUGGESTED_THREADS = ROLLOUT_SUGGESTED_THREADS;"
                             % (total, off_dx),
                             "const int ROLLOUT_FB_DYNAMIC_SHARED_MEM_COUNT = GRID_MAX_SOLVES_PER_BLOCK*(ROLLOUT_FB_LDS_PER_SOLVE + ROLLOUT_FB_OUT_PER_SOLVE);"])


def gen_rollout_feedback_control_device(self, use_thread_group=False):
    n = self.model.n
    self.gen_add_func_doc("The torque limits of the closed-loop rollout: v < lo ? lo : (v > hi ? hi : v), with a NaN v left as it is",
                          ["the library is compiled with -ffinite-math-only, under which the compiler may turn the two selects into min / max instructions that return the bound",
                           "for a NaN v; the NaN test therefore runs on the bit pattern, which no floating-point assumption touches: a diverged solve remains visible"],
                          ["v is the unclamped control", "lo is the lower limit", "hi is the upper limit"], "the applied control")
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__host__ __device__ __forceinline__")
    self.gen_add_code_line("T grid_clamp_keep_nan(const T v, const T lo, const T hi) {", True)
    self.gen_add_code_line("bool is_nan;")
    self.gen_add_code_line("if constexpr (sizeof(T) == 4) { unsigned int b; __builtin_memcpy(&b, &v, 4); is_nan = (b & 0x7fffffffu) > 0x7f800000u; }")
    self.gen_add_code_line("else { unsigned long long b; __builtin_memcpy(&b, &v, 8); is_nan = (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }")
    self.gen_add_code_line("const T c = v < lo ? lo : (v > hi ? hi : v);")
    self.gen_add_code_line("return is_nan ? v : c;")
    self.gen_add_end_function()
    self.gen_add_func_doc("The control of one closed-loop step in LDS: u = clamp(u_ff + K (x - x_ref)) (lane-group cooperative)",
                          ["all lanes of the solve's lane group must call it; on return s_tau holds the applied control and s_dx = [q - q_ref | qd - qd_ref], visible to the group",
                           "summation order: ONE accumulator that starts from u_ff, columns c = 0 .. 2n-1 ascending, v = v + K[c*n + lane]*dx[c] (tests restate it in NumPy float32)",
                           "the clamp is v < u_min ? u_min : (v > u_max ? u_max : v), and a NaN v stays NaN (grid_clamp_keep_nan)",
                           "K is read from global memory straight into the multiply-adds: 2n independent loads per lane, the n joint lanes of a solve read n contiguous values per column"],
                          ["s_tau receives the applied control (NUM_JOINTS values in LDS)", "s_dx receives x - x_ref (2*NUM_JOINTS values in LDS)",
                           "s_q is the vector of joint positions in LDS", "s_qd is the vector of joint velocities in LDS",
                           "d_K_row is this solve's gain record of this step in global memory: n x 2n, K[col*n + row]",
                           "xref_q is x_ref[lane] of this step (the position half)", "xref_qd is x_ref[n + lane] of this step (the velocity half)",
                           "u_ff is the feedforward control of joint `lane` of this step",
                           "d_u_min, d_u_max are the torque limits (NUM_JOINTS values each in global memory), or both nullptr: no limits",
                           "lane is the caller's lane index inside the solve's lane group"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void rollout_feedback_control_device(T *s_tau, T *s_dx, const T *s_q, const T *s_qd, const T *d_K_row, const T xref_q, const T xref_qd, const T u_ff, "
                           "const T *d_u_min, const T *d_u_max, const int lane) {", True)
    self.gen_add_code_line("T r_K[%d]; T r_lo = static_cast<T>(0), r_hi = static_cast<T>(0);" % (2 * n))
    self.gen_add_code_line("if (lane < %d) { // every load is issued before the first use: one exposed latency per step" % n, True)
    self.gen_add_code_line("#pragma unroll")
    self.gen_add_code_line("for (int c = 0; c < %d; c++) { r_K[c] = d_K_row[c*%d + lane]; }" % (2 * n, n))
    self.gen_add_code_line("if (d_u_min != nullptr) { r_lo = d_u_min[lane]; r_hi = d_u_max[lane]; }")
    self.gen_add_code_line("s_dx[lane] = s_q[lane] - xref_q; s_dx[%d + lane] = s_qd[lane] - xref_qd;" % n)
    self.gen_add_end_control_flow()
    self.gen_add_sync(use_thread_group)
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_line("T v = u_ff;")
    self.gen_add_code_line("#pragma unroll")
    self.gen_add_code_line("for (int c = 0; c < %d; c++) { v = v + r_K[c]*s_dx[c]; }" % (2 * n))
    self.gen_add_code_line("if (d_u_min != nullptr) { v = grid_clamp_keep_nan(v, r_lo, r_hi); }")
    self.gen_add_code_line("s_tau[lane] = v;")
    self.gen_add_end_control_flow()
    self.gen_add_sync(use_thread_group)
    self.gen_add_end_function()


def gen_rollout_feedback_kernel(self, use_thread_group=False, single_call_timing=False):
    n = self.model.n
    func_params = ["d_traj is the state trajectory (NUM_STEPS+1, NUM_TIMESTEPS, 2n), row 0 is x0, or nullptr",
                   "d_xT is the final state (NUM_TIMESTEPS, 2n), or nullptr",
                   "d_u_out is the applied control (NUM_STEPS, NUM_TIMESTEPS, n), after the limits, or nullptr",
                   "d_x0 is the initial state: the first 2n values of every row are [q | qd]",
                   "stride_x0 is the stride between the rows of d_x0 (>= 2n)",
                   "d_u is the feedforward control u_ff: element (t, k, j) at d_u[t*stride_u_step + k*stride_u_solve + j]",
                   "stride_u_step is the stride between the steps of d_u",
                   "stride_u_solve is the stride between the solves of d_u (0: every solve follows the same sequence)",
                   "d_K is the gain: element (t, k, c*n + j) at d_K[t*stride_K_step + k*stride_K_solve + c*n + j]",
                   "stride_K_step is the stride between the steps of d_K (0: one gain for all steps)",
                   "stride_K_solve is the stride between the solves of d_K (0: one gain for all solves)",
                   "d_xref is the reference: element (t, k, i), i < 2n, at d_xref[t*stride_xref_step + k*stride_xref_solve + i]",
                   "stride_xref_step is the stride between the steps of d_xref (0: a set point)",
                   "stride_xref_solve is the stride between the solves of d_xref (0: one reference for all solves)",
                   "d_u_min, d_u_max are the torque limits, n values each, shared by all solves and steps, or both nullptr",
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU (XImats, topology_helpers, etc.)",
                   "dt is the time step", "gravity is the gravity constant",
                   "NUM_TIMESTEPS is the number of independent solves (trajectories)",
                   "NUM_STEPS is the number of steps every solve takes"]
    func_def = "void rollout_feedback_kernel(T *d_traj, T *d_xT, T *d_u_out, const T *d_x0, const int stride_x0, const T *d_u, const long stride_u_step, const int stride_u_solve, " \
               "const T *d_K, const long stride_K_step, const int stride_K_solve, const T *d_xref, const long stride_xref_step, const int stride_xref_solve, " \
               "const T *d_u_min, const T *d_u_max, const robotModel<T> *d_robotModel, const T dt, const T gravity, const int NUM_TIMESTEPS, const int NUM_STEPS) {"
    notes = ["q and qd stay in the solve's LDS slice for all NUM_STEPS steps; the step loop is a runtime loop around ONE copy of the law and ONE copy of the (fully unrolled) aba_inner",
             "u_ff and x_ref of step t+1 are loaded into three registers before the dynamics of step t (their HBM latency hides behind the step; no fixture spills for them in fp32)",
             "K of step t is loaded inside the law of step t (one exposed latency per step; holding it across the dynamics would cost 2n registers per lane)",
             "K and x_ref are addressed as a wave-uniform 64-bit step base + a 32-bit offset rebuilt every step: no pointer is kept alive across the dynamics",
             "u_out[t] leaves through the head of the wave's staging; every row offset is 64-bit",
             "lane groups past the end of the batch walk the loop on the last solve's data and store nothing"]
    if single_call_timing:
        func_def = func_def.replace("kernel(", "kernel_single_timing(")
        notes = ["one solve (record 0) on the first lane group: NUM_TIMESTEPS is ignored, d_traj is (NUM_STEPS+1, 2n), d_xT (2n), d_u_out (NUM_STEPS, n); K, x_ref and u_ff are those of solve 0"]
    self.gen_add_func_doc("Roll NUM_TIMESTEPS independent trajectories forward by NUM_STEPS closed-loop steps: u = clamp(u_ff + K (x - x_ref)), ABA forward dynamics, semi-implicit Euler",
                          notes, func_params, None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__global__ GRID_LAUNCH_BOUNDS")
    self.gen_add_code_line(func_def, True)
    self.gen_kernel_prologue("ROLLOUT_FB_LDS_PER_SOLVE")
    self.gen_add_code_lines(["T *s_x = &s_mem[GRID_OFF_IN]; T *s_x0 = s_x; T *s_q = s_x; T *s_qd = &s_x[%d]; T *s_tau = &s_x[%d]; T *s_qdd = &s_mem[ROLLOUT_OFF_QDD]; T *s_dx = &s_mem[ROLLOUT_FB_OFF_DX];" % (n, 2 * n),
                             "T *s_out = &s_out_all[grp*%d];" % (2 * n),
                             "// the u_out row of the wave's solves is staged contiguously at the head of the wave's staging (n values per solve inside the 2n each one owns)",
                             "T *s_uo = &s_out_all[(grp & ~(GRID_SOLVES_PER_WAVE-1))*%d + (grp & (GRID_SOLVES_PER_WAVE-1))*%d];" % (2 * n, n)])
    gen_rollout_kernel_head(self, [("row", 2 * n), ("uo", n)], "d_traj, d_u_out", single_call_timing, use_thread_group, valid_unused=True)
    kk = "kc" if single_call_timing else "(k < NUM_TIMESTEPS ? k : NUM_TIMESTEPS - 1)"
    gen_rollout_load_x0(self, use_thread_group)  # (s_tau holds u_ff of step 0 until the law of step 0 overwrites it)
    self.gen_add_code_line("T r_xq = static_cast<T>(0), r_xv = static_cast<T>(0); // x_ref of step 0")
    self.gen_add_code_line("if (NUM_STEPS > 0 && lane < %d) { const int xo = kc*stride_xref_solve + lane; r_xq = d_xref[xo]; r_xv = d_xref[xo + %d]; }" % (n, n))
    save_row = lambda row_ptr_expr, name: gen_rollout_save(self, row_ptr_expr, name, 2 * n, "s_out", single_call_timing, use_thread_group, "s_x")
    self.gen_add_code_line("if (d_traj != nullptr) { // row 0 is x0", True)
    save_row("d_traj", "traj_t")
    self.gen_add_end_control_flow()
    gen_rollout_step_loop(self)
    self.gen_add_code_line("// the law of step t on the state in LDS; K_t comes straight from global memory (wave-uniform 64-bit step base + 32-bit offset)")
    self.gen_add_code_line("{ const T *d_K_t = d_K + static_cast<long>(t)*stride_K_step; const int ko = %s*stride_K_solve;" % kk, True)
    self.gen_add_code_line("rollout_feedback_control_device<T>(s_tau, s_dx, s_q, s_qd, d_K_t + ko, r_xq, r_xv, r_u, d_u_min, d_u_max, lane);")
    self.gen_add_end_control_flow()
    self.gen_add_code_line("if (d_u_out != nullptr) {", True)
    gen_rollout_save(self, "d_u_out + static_cast<size_t>(t)*uo_stride", "uo_t", n, "s_uo", single_call_timing, use_thread_group, "s_tau")
    self.gen_add_end_control_flow()

    self.gen_add_code_line("// u_ff and x_ref of the next step leave for the registers now and are used by the law after this step's dynamics")
    self.gen_add_code_line("// (wave-uniform 64-bit step bases + 32-bit lane offsets, rebuilt from k every step: no pointer is kept alive across the ABA)")
    gen_rollout_prefetch_control(self, single_call_timing)
    self.gen_add_code_line("r_xq = static_cast<T>(0); r_xv = static_cast<T>(0);")
    self.gen_add_code_line("if (t + 1 < NUM_STEPS && lane < %d) { const T *d_xref_t = d_xref + static_cast<long>(t + 1)*stride_xref_step; const int xo = %s*stride_xref_solve + lane; r_xq = d_xref_t[xo]; r_xv = d_xref_t[xo + %d]; }"
                           % (n, kk, n))
    self.gen_add_code_line("rollout_device<T>(s_q, s_qd, s_tau, s_qdd, s_mem, d_robotModel, dt, gravity, lane);")
    self.gen_add_code_line("if (d_traj != nullptr) {", True)
    save_row("d_traj + static_cast<size_t>(t + 1)*row_stride", "traj_t")
    self.gen_add_end_control_flow()
    self.gen_add_end_control_flow()
    self.gen_add_code_line("if (d_xT != nullptr) {", True)
    save_row("d_xT", "xT_k")
    self.gen_add_end_control_flow()
    if not single_call_timing:
        self.gen_add_end_control_flow()
    self.gen_add_end_function()


ROLLOUT_FEEDBACK_RESERVE = dict(
    name="rollout_feedback", base="rollout", min_steps=0,
    doc=("Reserves the buffers of the closed-loop rollout for num_timesteps solves of num_steps steps (those of rollout_reserve, the gains, the reference, the applied control and the limits)",
         ["d_K_traj / h_K_traj: (num_steps, num_timesteps, 2n^2), records K[c*n + j]; d_xref_traj / h_xref_traj: (num_steps, num_timesteps, 2n); d_uout_traj / h_uout_traj: (num_steps, num_timesteps, n);",
          "d_u_lim / h_u_lim: 2n values, u_min | u_max.  Null after init_gridData; the rollout_feedback host wrappers call this themselves, a caller calls it first to get the h_ buffers to fill; grows on demand, close_grid frees"]),
    rows=[("K_traj", "2*NUM_JOINTS*NUM_JOINTS", "(S > 0 ? S : 1)*N"), ("xref_traj", "2*NUM_JOINTS", "(S > 0 ? S : 1)*N"), ("uout_traj", "NUM_JOINTS", "(S > 0 ? S : 1)*N"),
          ("u_lim", "2*NUM_JOINTS", "1")])

ROLLOUT_FEEDBACK_HOST = dict(
    name="rollout_feedback", tag="ROLLOUT_FB", x0=True,
    doc=("Roll num_timesteps trajectories forward by num_steps closed-loop steps (u = clamp(u_ff + K (x - x_ref)), ABA forward dynamics, semi-implicit Euler)",
         ["no counterpart in the reference; call rollout_feedback_reserve first and fill h_u_traj (u_ff), h_K_traj, h_xref_traj and, with use_limits, h_u_lim (u_min | u_max)",
          "_single_timing: solve 0 alone, num_steps steps in one launch, time per step printed; h_x_traj holds its (num_steps+1, 2n) trajectory, h_uout_traj its (num_steps, n) controls"],
         "x0 in h_q_qd_u (rows of 3n, [q | qd | unused]), u_ff in h_u_traj (num_steps, num_timesteps, n), K in h_K_traj (num_steps, num_timesteps, 2n^2), x_ref in h_xref_traj "
         "(num_steps, num_timesteps, 2n), limits in h_u_lim (2n); results in h_x_traj (num_steps+1, num_timesteps, 2n) and h_uout_traj (num_steps, num_timesteps, n)", "takes"),
    extra_params=[("const bool use_limits", "use_limits says that h_u_lim is filled: the control is clamped to [u_min, u_max]")],
    setup=["const int stride_K_solve = 2*NUM_JOINTS*NUM_JOINTS; const long stride_K_step = static_cast<long>(stride_K_solve)*%(N)s; "
           "const int stride_xref_solve = 2*NUM_JOINTS; const long stride_xref_step = static_cast<long>(stride_xref_solve)*%(N)s;",
           "const T *d_u_min = use_limits ? hd_data->d_u_lim : static_cast<const T *>(nullptr); const T *d_u_max = use_limits ? hd_data->d_u_lim + NUM_JOINTS : static_cast<const T *>(nullptr);"],
    args="hd_data->d_x_traj,static_cast<T *>(nullptr),hd_data->d_uout_traj,hd_data->d_q_qd_u,stride_x0,hd_data->d_u_traj,stride_u_step,stride_u_solve,"
         "hd_data->d_K_traj,stride_K_step,stride_K_solve,hd_data->d_xref_traj,stride_xref_step,stride_xref_solve,d_u_min,d_u_max,d_robotModel,dt,gravity,num_timesteps,num_steps);",
    h2d=[("q_qd_u", "stride_x0", ""), ("u_traj", "NUM_JOINTS", "*num_steps"), ("K_traj", "2*NUM_JOINTS*NUM_JOINTS", "*num_steps"), ("xref_traj", "2*NUM_JOINTS", "*num_steps"),
         ("u_lim", "2*NUM_JOINTS", "", "1")],
    d2h=[("x_traj", "2*NUM_JOINTS", "*(num_steps + 1)"), ("uout_traj", "NUM_JOINTS", "*num_steps")])


def gen_rollout_feedback_reserve(self):
    gen_rollout_family_reserve(self, ROLLOUT_FEEDBACK_RESERVE)


def gen_rollout_feedback_host(self, mode=0):
    gen_rollout_family_host(self, ROLLOUT_FEEDBACK_HOST, mode)


def gen_rollout_feedback(self, use_thread_group=False):
    self.gen_rollout_feedback_constants()
    self.gen_rollout_feedback_control_device(use_thread_group)
    self.gen_rollout_feedback_kernel(use_thread_group, True)
    self.gen_rollout_feedback_kernel(use_thread_group, False)
    self.gen_rollout_feedback_reserve()
    for mode in (0, 1, 2):
        self.gen_rollout_feedback_host(mode)
