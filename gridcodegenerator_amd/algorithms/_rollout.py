"""Fused multi-step rollout (ABA forward dynamics + semi-implicit Euler), emitter for the HIP/CDNA4 backend.

The reference has no counterpart: every algorithm it emits answers "what is X at each of these states"; none advances a state.  A stepwise
rollout built from them is T dependent launches of aba_kernel with the state going out to HBM and back between them.  Here one launch keeps
q and qd of every solve in its LDS slice for all T steps, reads one control row and (optionally) writes one state row per step.

Semantics, per solve k and step t = 0 .. T-1 (no joint limits, no angle wrapping, no contact):
    qdd      = ABA(q_t, qd_t, u_t)            aba_device: gravity convention and damping of aba_kernel
    qd_{t+1} = qd_t + dt*qdd
    q_{t+1}  = q_t  + dt*qd_{t+1}             the NEW velocity (symplectic Euler)
Both update lines live in grid_symplectic_euler_step and nowhere else.

Layouts (time-major, so that what one wave moves per step is one contiguous span):
    x0    (N, stride_x0)  the first 2n values of a row are [q | qd]
    u     element (t, k, j) at d_u[t*stride_u_step + k*stride_u_solve + j]; stride_u_solve == 0 shares one sequence between all solves
    traj  (T+1, N, 2n)    row 0 is x0 (optional)
    xT    (N, 2n)         the final state (optional)
The lane groups of a wave own consecutive solves, so row t of a wave is written by the wave-cooperative saver of every other kernel
(gen_kernel_save_result) with the row's base pointer in place of the output's.

LDS: the slice of aba_kernel as it is: q | qd | u sit in GRID_OFF_IN and qdd goes into its spare fourth slot; the staging record is [q | qd].
"""
from ._rollout_common import gen_rollout_commit_control, gen_rollout_family_host, gen_rollout_family_reserve, gen_rollout_kernel_head, gen_rollout_load_x0, \
    gen_rollout_prefetch_control, gen_rollout_save, gen_rollout_step_loop


def gen_rollout_constants(self):
    n = self.model.n
    K = self.gen_lds_layout()["KERNELS"]["ABA"]
    self.gen_add_code_line("//")
    self.gen_add_code_line("// rollout: T steps of aba + symplectic Euler in one launch.  Slice: the one of aba (qdd in the spare slot of GRID_OFF_IN); staging: one [q | qd] row per solve")
    self.gen_add_code_line("//")
    self.gen_add_code_lines(["const int ROLLOUT_LDS_PER_SOLVE = ABA_LDS_PER_SOLVE; const int ROLLOUT_OUT_PER_SOLVE = %d; const int ROLLOUT_OFF_QDD = GRID_OFF_IN + %d; const int ROLLOUT_SUGGESTED_THREADS = ABA_SUGGESTED_THREADS;"
                             % ((2 * n + 3) // 4 * 4, 3 * n),
                             "const int ROLLOUT_DYNAMIC_SHARED_MEM_COUNT = GRID_MAX_SOLVES_PER_BLOCK*(ROLLOUT_LDS_PER_SOLVE + ROLLOUT_OUT_PER_SOLVE);"])
    assert K["LDS"] >= self.gen_lds_layout()["IN"] + 4 * n  # (the qdd slot lies inside the prefix aba carves)


def gen_rollout_step_helper(self):
    self.gen_add_func_doc("One semi-implicit (symplectic) Euler update of one joint",
                          ["the only place the integrator is written down: qd += dt*qdd, then q += dt*qd with the NEW velocity"],
                          ["q is the joint position (updated)", "qd is the joint velocity (updated)", "qdd is the joint acceleration", "dt is the step"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__host__ __device__ __forceinline__")
    self.gen_add_code_line("void grid_symplectic_euler_step(T &q, T &qd, const T qdd, const T dt) {", True)
    self.gen_add_code_line("qd = qd + dt*qdd;")
    self.gen_add_code_line("q = q + dt*qd;")
    self.gen_add_end_function()


def gen_rollout_device(self, use_thread_group=False):
    n = self.model.n
    self.gen_add_func_doc("One rollout step in LDS: aba_device, then the symplectic Euler update of (q, qd) (lane-group cooperative)",
                          ["all lanes of the solve's lane group must call it; the new s_q, s_qd (and the step's s_qdd) are visible to the group on return"],
                          ["s_q is the vector of joint positions in LDS (updated)", "s_qd is the vector of joint velocities in LDS (updated)",
                           "s_tau is the vector of joint torques of this step in LDS", "s_qdd receives the joint accelerations of this step",
                           "s_work is this solve's LDS workspace of ROLLOUT_LDS_PER_SOLVE elements",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU", "dt is the time step", "gravity is the gravity constant",
                           "lane is the caller's lane index inside the solve's lane group"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void rollout_device(T *s_q, T *s_qd, const T *s_tau, T *s_qdd, T *s_work, const robotModel<T> *d_robotModel, const T dt, const T gravity, const int lane) {", True)
    self.gen_add_code_line("aba_device<T>(s_qdd, s_q, s_qd, s_tau, s_work, d_robotModel, gravity, lane);")
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_line("T q = s_q[lane]; T qd = s_qd[lane];")
    self.gen_add_code_line("grid_symplectic_euler_step(q, qd, s_qdd[lane], dt);")
    self.gen_add_code_line("s_qd[lane] = qd; s_q[lane] = q;")
    self.gen_add_end_control_flow()
    self.gen_add_sync(use_thread_group)  # (the next step's X(q) update and aba_inner read s_q / s_qd on every lane)
    self.gen_add_end_function()


def gen_rollout_kernel(self, use_thread_group=False, single_call_timing=False):
    n = self.model.n
    func_params = ["d_traj is the state trajectory (NUM_STEPS+1, NUM_TIMESTEPS, 2n), row 0 is x0, or nullptr: nothing is written during the loop",
                   "d_xT is the final state (NUM_TIMESTEPS, 2n), or nullptr",
                   "d_x0 is the initial state: the first 2n values of every row are [q | qd]",
                   "stride_x0 is the stride between the rows of d_x0 (>= 2n)",
                   "d_u is the control: element (t, k, j) at d_u[t*stride_u_step + k*stride_u_solve + j]",
                   "stride_u_step is the stride between the steps of d_u",
                   "stride_u_solve is the stride between the solves of d_u (0: every solve follows the same sequence)",
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU (XImats, topology_helpers, etc.)",
                   "dt is the time step", "gravity is the gravity constant",
                   "NUM_TIMESTEPS is the number of independent solves (trajectories)",
                   "NUM_STEPS is the number of steps every solve takes"]
    func_def = "void rollout_kernel(T *d_traj, T *d_xT, const T *d_x0, const int stride_x0, const T *d_u, const long stride_u_step, const int stride_u_solve, " \
               "const robotModel<T> *d_robotModel, const T dt, const T gravity, const int NUM_TIMESTEPS, const int NUM_STEPS) {"
    notes = ["q and qd stay in the solve's LDS slice for all NUM_STEPS steps; the step loop is a runtime loop around ONE copy of the (fully unrolled) aba_inner",
             "the control of step t+1 is loaded into a register before the ABA of step t (its HBM latency hides behind the step)",
             "lane groups past the end of the batch walk the loop on the last solve's data and store nothing"]
    if single_call_timing:
        func_def = func_def.replace("kernel(", "kernel_single_timing(")
        notes = ["one solve (record 0) on the first lane group: NUM_TIMESTEPS is ignored, d_traj is (NUM_STEPS+1, 2n) and d_xT is (2n)"]
    self.gen_add_func_doc("Roll NUM_TIMESTEPS independent trajectories forward by NUM_STEPS steps of ABA forward dynamics + semi-implicit Euler", notes, func_params, None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__global__ GRID_LAUNCH_BOUNDS")
    self.gen_add_code_line(func_def, True)
    self.gen_kernel_prologue("ROLLOUT_LDS_PER_SOLVE")
    self.gen_add_code_lines(["T *s_x = &s_mem[GRID_OFF_IN]; T *s_x0 = s_x; T *s_q = s_x; T *s_qd = &s_x[%d]; T *s_tau = &s_x[%d]; T *s_qdd = &s_mem[ROLLOUT_OFF_QDD];" % (n, 2 * n),
                             "T *s_out = &s_out_all[grp*%d];" % (2 * n)])
    gen_rollout_kernel_head(self, [("row", 2 * n)], "d_traj", single_call_timing, use_thread_group)
    gen_rollout_load_x0(self, use_thread_group)
    save_row = lambda row_ptr_expr, name: gen_rollout_save(self, row_ptr_expr, name, 2 * n, "s_out", single_call_timing, use_thread_group, "s_x")
    self.gen_add_code_line("if (d_traj != nullptr) { // row 0 is x0", True)
    save_row("d_traj", "traj_t")
    self.gen_add_end_control_flow()
    gen_rollout_step_loop(self)
    self.gen_add_code_line("// the next step's control leaves for the registers now and lands in LDS after this step")
    self.gen_add_code_line("// (wave-uniform 64-bit step base + 32-bit lane offset, rebuilt from k every step: no pointer is kept alive across the ABA)")
    gen_rollout_prefetch_control(self, single_call_timing)
    self.gen_add_code_line("rollout_device<T>(s_q, s_qd, s_tau, s_qdd, s_mem, d_robotModel, dt, gravity, lane);")
    gen_rollout_commit_control(self, use_thread_group)
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


ROLLOUT_RESERVE = dict(
    name="rollout", base=None, min_steps=0,
    doc=("Reserves the rollout buffers of hd_data for num_timesteps solves of num_steps steps (the reference's gridData has no such buffers)",
         ["d_u_traj / h_u_traj: the control (num_steps, num_timesteps, n); d_x_traj / h_x_traj: the states (num_steps+1, num_timesteps, 2n)",
          "null after init_gridData; the rollout host wrappers call this themselves, a caller calls it first to get h_u_traj to fill; grows on demand, close_grid frees"]),
    rows=[("u_traj", "NUM_JOINTS", "(S > 0 ? S : 1)*N"), ("x_traj", "2*NUM_JOINTS", "(S + 1)*N")])

ROLLOUT_HOST = dict(
    name="rollout", tag="ROLLOUT", x0=True,
    doc=("Roll num_timesteps trajectories forward by num_steps steps (ABA forward dynamics + semi-implicit Euler)",
         ["no counterpart in the reference; call rollout_reserve first and fill h_u_traj",
          "_single_timing: solve 0 alone, num_steps steps in one launch, time per step printed; h_x_traj holds its (num_steps+1, 2n) trajectory"],
         "x0 in h_q_qd_u (rows of 3n, [q | qd | unused]), u in h_u_traj (num_steps, num_timesteps, n), result in h_x_traj (num_steps+1, num_timesteps, 2n)", "takes"),
    args="hd_data->d_x_traj,static_cast<T *>(nullptr),hd_data->d_q_qd_u,stride_x0,hd_data->d_u_traj,stride_u_step,stride_u_solve,d_robotModel,dt,gravity,num_timesteps,num_steps);",
    h2d=[("q_qd_u", "stride_x0", ""), ("u_traj", "NUM_JOINTS", "*num_steps")],
    d2h=[("x_traj", "2*NUM_JOINTS", "*(num_steps + 1)")])


def gen_rollout_reserve(self):
    gen_rollout_family_reserve(self, ROLLOUT_RESERVE)


def gen_rollout_host(self, mode=0):
    gen_rollout_family_host(self, ROLLOUT_HOST, mode)


def gen_rollout(self, use_thread_group=False):
    self.gen_rollout_constants()
    self.gen_rollout_step_helper()
    self.gen_rollout_device(use_thread_group)
    self.gen_rollout_kernel(use_thread_group, True)
    self.gen_rollout_kernel(use_thread_group, False)
    self.gen_rollout_reserve()
    for mode in (0, 1, 2):
        self.gen_rollout_host(mode)
