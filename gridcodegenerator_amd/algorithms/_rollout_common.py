"""The skeleton the rollout family shares (rollout, rollout_linearized, rollout_adjoint, rollout_feedback), emitter helpers for the HIP/CDNA4 backend.

Every member is one kernel that keeps a solve's state in its LDS slice for NUM_STEPS steps, a *_reserve function for its gridData buffers and three host wrappers
(plain, _single_timing, _compute_only).  What differs between the members in substance - the step functions and the bodies of the step loops - stays in their own
modules.  What is here: the head of the kernel (one solve on the first lane group, or the batch loop, with the strides between two time slices), the step loop's
opening, the control prefetch of the forward members, the row saver, and the reserve / host emitters, the last two driven by a small description (ROLLOUT_HOST,
ROLLOUT_RESERVE in _rollout.py are the shortest examples).  A new member supplies its constants, its step function, its loop body and those two descriptions.
"""


def _pad4(x):
    return (x + 3) // 4 * 4


def gen_rollout_kernel_head(self, strides, slices, single_call_timing, use_thread_group, valid_unused=False):
    """Opens the solve: record 0 on the first lane group (single_call_timing), or the batch loop over k (left open: the caller closes it).
    strides: [(name, values per solve)] -> `const size_t <name>_stride`, the elements between two time slices of the buffers `slices` names.
    (One stride shares the line of the code around it, several get a line of their own.)"""
    if single_call_timing:
        head = "const int k = 0; const int kc = 0; const bool valid = (blockIdx.x + blockIdx.y == 0) && (grp == 0); const int lane = lane_id;"
        consts = " ".join("const size_t %s_stride = %d;" % s for s in strides)
        if len(strides) == 1:
            self.gen_add_code_line(head + " " + consts + " (void)k; (void)NUM_TIMESTEPS;")
        else:
            self.gen_add_code_line(head + " (void)k; (void)NUM_TIMESTEPS;")
            self.gen_add_code_line(consts)
        self.gen_add_code_line("if (!valid) {return;}")
    else:
        self.gen_add_parallel_loop("k", "NUM_TIMESTEPS", use_thread_group, block_level=True)
        consts = " ".join("const size_t %s_stride = static_cast<size_t>(NUM_TIMESTEPS)*%d;" % s for s in strides)
        if len(strides) == 1:
            self.gen_add_code_line(consts + " // elements between two time slices of " + slices)
        else:
            self.gen_add_code_line("// elements between two time slices of " + slices)
            self.gen_add_code_line(consts + (" (void)valid;" if valid_unused else ""))


def gen_rollout_step_loop(self, reverse=False):
    """Opens the step loop (left open: the caller closes it) with the opaque lane index every step body uses."""
    self.gen_add_code_line("for (int t = NUM_STEPS - 1; t >= 0; t--){" if reverse else "for (int t = 0; t < NUM_STEPS; t++){", True)
    self.gen_add_code_line("const int lane = grid_loop_variant(lane_id); // (shadows the outer one: keeps lane-dependent values from being hoisted out of the step loop and spilled)")


def gen_rollout_commit_control(self, use_thread_group):
    """The control that was prefetched into r_u lands in LDS."""
    self.gen_add_code_line("if (lane < %d) { s_tau[lane] = r_u; }" % self.model.n)
    self.gen_add_sync(use_thread_group)


def gen_rollout_load_x0(self, use_thread_group):
    """x0 and the control of step 0 into the slice (forward members)."""
    n = self.model.n
    self.gen_add_code_line("T r_u = (NUM_STEPS > 0 && lane < %d) ? d_u[kc*stride_u_solve + lane] : static_cast<T>(0); // control of step 0, in flight while x0 arrives" % n)
    self.gen_kernel_load_inputs("x0", "stride_x0", 2 * n, use_thread_group)
    gen_rollout_commit_control(self, use_thread_group)


def gen_rollout_prefetch_control(self, single_call_timing):
    """Requests the control of step t+1 before the dynamics of step t (forward members); gen_rollout_commit_control stores it after the step."""
    self.gen_add_code_line("const T *d_u_t = d_u + static_cast<long>(t + 1)*stride_u_step;")
    self.gen_add_code_line("r_u = (t + 1 < NUM_STEPS && lane < %d) ? d_u_t[%s*stride_u_solve + lane] : static_cast<T>(0);"
                           % (self.model.n, "kc" if single_call_timing else "(k < NUM_TIMESTEPS ? k : NUM_TIMESTEPS - 1)"))


def gen_rollout_save(self, row_ptr_expr, name, amount, src, single_call_timing, use_thread_group, copy_from=None):
    """Stores the wave's records of `amount` values (staged at `src`, contiguous over the wave's lane groups) to `row_ptr_expr` (a T* to record 0 of the time slice)
    with the wave-cooperative saver of every other kernel; copy_from: LDS vector staged into src first."""
    if not single_call_timing:
        # the saver's addresses and counts depend on tid, grp and k alone: invariants that LLVM hoists out of the step loop (and out of the batch loop) and
        # keeps in VGPRs across the dynamics (chain12, 245 VGPRs in aba_kernel, then spills).  Opaque copies make it rebuild them per row: a handful of integer instructions.
        self.gen_add_code_line("const int tid_t = grid_loop_variant(tid); const int grp_t = grid_loop_variant(grp); const int k_t = grid_loop_variant(k);")
        self.gen_add_code_line("{ const int tid = tid_t; const int grp = grp_t; const int k = k_t; (void)tid; // (shadow the invariants)", True)
    else:
        self.gen_add_code_line("{", True)
    self.gen_add_code_line("T *d_%s = %s;" % (name, row_ptr_expr))
    if copy_from is not None:
        self.gen_add_parallel_loop("ind", str(amount), use_thread_group)
        self.gen_add_code_line("%s[ind] = %s[ind];" % (src, copy_from))
        self.gen_add_end_control_flow()
    if single_call_timing:
        self.gen_kernel_save_result_single_timing(name, amount, use_thread_group, src)
        self.gen_add_sync(use_thread_group)
    else:
        self.gen_kernel_save_result(name, amount, amount, use_thread_group, src)
    self.gen_add_end_control_flow()


def gen_rollout_family_reserve(self, desc):
    """desc: name, doc (summary, notes), base (the *_reserve called first, or None), min_steps (what S is without a step: 0 or 1) and
    rows [(gridData field, values per record, records)] in terms of N and S."""
    self.gen_add_func_doc(desc["doc"][0], desc["doc"][1],
                          ["hd_data is the packaged input and output pointers", "num_timesteps is the number of solves", "num_steps is the number of steps"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__host__")
    self.gen_add_code_line("void %s_reserve(gridData<T> *hd_data, const int num_timesteps, const int num_steps) {" % desc["name"], True)
    if desc["base"]:
        self.gen_add_code_line("%s_reserve<T>(hd_data, num_timesteps, num_steps);" % desc["base"])
    self.gen_add_code_line("const int N = num_timesteps > 1 ? num_timesteps : 1; const int S = num_steps > 0 ? num_steps : %d;" % desc["min_steps"])
    for field, per, count in desc["rows"]:
        self.gen_add_code_line("grid_ee_reserve<T>(&hd_data->d_%s, &hd_data->h_%s, %s, %s);" % (field, field, per, count))
    self.gen_add_end_function()


def gen_rollout_family_host(self, desc, mode):
    """One host wrapper of a member: mode 0 = H2D, launch, D2H; 1 = _single_timing (solve 0 alone, time per step printed); 2 = _compute_only (the launch alone).
    desc: name, tag (prefix of the member's constants and of the printf), doc (summary, notes of mode 0, what hd_data holds, "takes" / "took"),
    x0 (True where the kernel takes stride_x0), args (the kernel's arguments, as the launch spells them) and
    h2d / d2h rows [(gridData field, values per solve, factor over the steps)]; a row with a fourth entry is not per solve: the entry is its whole count.
    Optional: extra_params [(C++ parameter, its doc line)] that follow num_steps, setup (lines behind the strides; %(N)s is the number of solves of this mode)."""
    single_call_timing = mode == 1
    compute_only = mode == 2
    summary, notes, hd_data, takes = desc["doc"]
    func_params = ["hd_data is the packaged input and output pointers: " + hd_data,
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU (XImats, topology_helpers, etc.)",
                   "dt is the time step", "gravity is the gravity constant,",
                   "num_timesteps is the number of independent solves (trajectories)", "num_steps is the number of steps every solve " + takes]
    func_params += [doc for _, doc in desc.get("extra_params", [])]
    func_params += ["streams are pointers to HIP streams for async memory transfers (if needed)"]
    suffix = ("_single_timing" if single_call_timing else "") + ("_compute_only" if compute_only else "")
    self.gen_add_func_doc(summary, notes if mode == 0 else [], func_params, None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__host__")
    self.gen_add_code_line("void " + desc["name"] + suffix + "(gridData<T> *hd_data, const robotModel<T> *d_robotModel, const T dt, const T gravity, const int num_timesteps, const int num_steps,"
                           + "".join(" %s," % p for p, _ in desc.get("extra_params", [])))
    self.gen_add_code_line("                      const dim3 block_dimms, const dim3 thread_dimms" + ("" if compute_only else ", hipStream_t *streams") + ") {", True)
    N = "1" if single_call_timing else "num_timesteps"
    copy = lambda row, dst, src, tail: "gpuErrchk(hipMemcpy%s(hd_data->%s_%s,hd_data->%s_%s,static_cast<size_t>(%s)*%s%s*sizeof(T),%s));" \
        % (("Async" if dst == "d" else ""), dst, row[0], src, row[0], row[1], N if len(row) < 4 else row[3], row[2], tail)
    self.gen_add_code_lines(["%s_reserve<T>(hd_data, %s, num_steps);" % (desc["name"], N),
                             ("const int stride_x0 = 3*NUM_JOINTS; " if desc["x0"] else "")
                             + "const int stride_u_solve = NUM_JOINTS; const long stride_u_step = static_cast<long>(NUM_JOINTS)*%s;" % N]
                            + [ln % {"N": N} for ln in desc.get("setup", [])])
    if not compute_only:
        self.gen_add_code_line("// start code with memory transfer")
        self.gen_add_code_lines([copy(row, "d", "h", "hipMemcpyHostToDevice,streams[0]") for row in desc["h2d"]])
        self.gen_add_code_line("gpuErrchk(hipDeviceSynchronize());")
    self.gen_add_code_line("// then call the kernel")
    if single_call_timing:
        self.gen_add_code_line("struct timespec start, end; clock_gettime(CLOCK_MONOTONIC,&start);")
    self.gen_add_code_lines(["hipLaunchKernelGGL((%s_kernel%s<T>),block_dimms,thread_dimms,grid_lds_bytes<T>(thread_dimms, %s_LDS_PER_SOLVE, %s_OUT_PER_SOLVE),0,%s"
                             % (desc["name"], "_single_timing" if single_call_timing else "", desc["tag"], desc["tag"], desc["args"]),
                             "gpuErrchk(hipGetLastError()); gpuErrchk(hipDeviceSynchronize());"])
    if single_call_timing:
        self.gen_add_code_line("clock_gettime(CLOCK_MONOTONIC,&end);")
    if not compute_only:
        self.gen_add_code_line("// finally transfer the result%s back" % ("s" if len(desc["d2h"]) > 1 else ""))
        self.gen_add_code_lines([copy(row, "h", "d", "hipMemcpyDeviceToHost") for row in desc["d2h"]])
        self.gen_add_code_line("gpuErrchk(hipDeviceSynchronize());")
    if single_call_timing:
        self.gen_add_code_line("printf(\"Single Call %s %%fus\\n\",time_delta_us_timespec(start,end)/static_cast<double>(num_steps > 0 ? num_steps : 1));" % desc["tag"])
    self.gen_add_end_function()
