"""Joint-space inertia matrix M(q) by the composite rigid body algorithm, emitter for the HIP/CDNA4 backend.

Keeps the reference's Python names (reference algorithms/_crba.py: gen_crba_inner :30, device :219, kernel :254, host :310,
gen_crba :377) and its emitted surface (crba_device / crba_kernel / crba host wrapper with the reference's arguments), but not its
inner: the reference's s_XImats offsets are hard-coded for a 7-joint arm (:107-140, "works for iiwa but not for hyq", :313).

Lane-group form (lane j <-> joint j, column j of M), one backward sweep over the tree in post-order:
  * lanes 0..5 own column c of every composite inertia I^C_i (initialised with the link inertia I_i); once joint i's subtree has been
    folded in, I^C_p += X_i^T I^C_i X_i is done as two one-sided products with a 6x6 transpose through LDS in between - the same
    code as direct_minv's backward sweep (gen_inertia_to_parent), without the U D^-1 U^T correction;
  * lane j carries F_i[:, j] = X_{i<-j}^T I^C_j S_j for every i on its root path (zero elsewhere): at joint j it takes F = I^C_j S_j
    (column S_j of I^C_j, broadcast from the lane that owns it) and the vector walks up with the sweep, F_p += X_i^T F_i;
  * M[i][j] = S_i^T F_i[:, j] for every ancestor-or-self i of j, exactly 0 for the other i (zeros propagate structurally).
Lane j then writes M[i][j] (i <= j) into both slots (i, j) and (j, i) of the dense record: every pair is computed once, so M is
exactly symmetric, and pairs where neither joint is an ancestor of the other are exact zeros.
M does not depend on gravity or on q_dot: the kernel reads the first n values of every input row.

Output layout (reference): d_M[k*n*n + col*n + row], dense (both triangles, structural zeros included); row- and column-major coincide.
"""


# Longest chain on which crba takes the tip-frame form.  Its frame scan keeps the whole chain in registers: on the 8- and 12-joint chains the
# T = double instantiation spills (20 and 556 bytes per lane; direct_minv_inner_tip itself spills 596 bytes on the 12-joint chain), so those
# chains take the column walk, which stays at 0 bytes of scratch in both precisions.
CRBA_TIP_MAX_L = 7


def crba_form(self):
    """"tip", "branch" or "walk": the formulation direct_minv uses for this robot (tip-frame chains up to CRBA_TIP_MAX_L joints), else the column walk"""
    if self.tip_frame and self.tip_L <= CRBA_TIP_MAX_L:
        return "tip"
    if self.branch_components:
        return "branch"
    return "walk"


def gen_crba_inner_temp_mem_size(self):
    return 0  # LDS needs are a prefix of the fixed per-solve slice (helpers/_topology_helpers.py: gen_lds_layout, KERNELS["CRBA"])


def gen_crba_device_temp_mem_size(self):
    return self.gen_lds_layout()["KERNELS"]["CRBA"]["LDS"]


def gen_crba_inner_function_call(self, use_thread_group=False, updated_var_names=None):
    if crba_form(self) == "tip":
        self.gen_add_code_line("crba_inner_tip<T>(s_M, s_X, &s_work[GRID_OFF_U], d_robotModel, lane);")
    elif crba_form(self) == "branch":
        self.gen_add_code_line("crba_inner_branch<T>(s_M, s_X, &s_work[off_sp], d_robotModel, lane);")
    else:
        self.gen_add_code_line("crba_inner<T>(s_M, s_X, s_T, d_robotModel, lane);")
    self.gen_add_sync(use_thread_group)


def gen_crba_inner(self, use_thread_group=False):
    """The inner of the formulation direct_minv uses for this robot, so that M and M^-1 of one library come from the same assembly:
    tip-frame robots crba_inner_tip (algorithms/_tip_frame_gradient.py), branch-component robots crba_inner_branch (the `crba` mode of
    algorithms/_branch_frame_gradient.py), every other robot - and tip-frame chains longer than CRBA_TIP_MAX_L - the column walk crba_inner below."""
    if crba_form(self) == "tip":
        self.gen_crba_inner_tip(use_thread_group)
        return
    if crba_form(self) == "branch":
        from ._branch_frame_gradient import _emit_branch_inner
        _emit_branch_inner(self, "crba", use_thread_group)
        return
    from ._direct_minv import gen_inertia_to_parent
    m = self.model
    n = m.n
    ld = self.minv_ld
    self.gen_add_func_doc("Compute the joint-space inertia matrix M(q) (dense, symmetric) into LDS by the composite rigid body algorithm",
                          ["lane j produces column j of M and, by symmetry, row j; lanes 0..5 also carry one column of every composite inertia",
                           "the caller must grid_wave_sync() before other lanes' entries of s_M are read"],
                          ["s_M is the n x n output in LDS (s_M[row*GRID_MINV_LD + col])",
                           "s_X is this solve's compact X(q) storage", "s_T is LDS scratch for the 6x6 transpose (two buffers of 40)",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU",
                           "lane is the caller's lane index inside the solve's lane group"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void crba_inner(T *s_M, const T *s_X, T *s_T, const robotModel<T> *d_robotModel, const int lane) {", True)
    self.gen_add_code_line("const int cI = lane < 5 ? lane : 5; // composite-inertia column owned by this lane (lanes 0..5 are live)")
    self.gen_add_code_line("const bool isIA = lane < 6;")
    self.gen_add_code_line("const T *d_I = &grid_model_constants(static_cast<const T *>(nullptr))[" + str(18 * n) + " + 6*cI]; (void)d_robotModel;")
    self.gen_add_code_line("T Mcol[" + str(n) + "];")
    self.gen_add_code_line("//")
    self.gen_add_code_line("// backward sweep (post-order): composite inertias I^C to the parent, F_i[:, lane] up the root path, M[i][lane] = S_i^T F_i")
    self.gen_add_code_line("//")

    def pre(i):
        self.gen_add_code_line("T IC_%d[6], F_%d[6];" % (i, i))
        self.gen_add_code_line("#pragma unroll")
        self.gen_add_code_line("for (int r = 0; r < 6; r++) { IC_%d[r] = d_I[%d + r]; F_%d[r] = static_cast<T>(0); }" % (i, 36 * i, i))

    def post(i):
        s, p = m.S_index[i], m.parent[i]
        self.gen_add_code_line("{", True)
        self.gen_add_code_line("// I^C_%d is complete: its column S lives in lane %d; lane %d starts its F there" % (i, s, i))
        self.gen_add_code_line("#pragma unroll")
        self.gen_add_code_line("for (int r = 0; r < 6; r++) { const T u = grid_group_shfl(IC_%d[r], %d); F_%d[r] += (lane == %d) ? u : static_cast<T>(0); }" % (i, s, i, i))
        self.gen_add_code_line("Mcol[%d] = F_%d[%d]; grid_pin(Mcol[%d]);" % (i, i, s, i))
        if p != -1:
            self.gen_add_code_line("T X[18]; grid_load_X(X, &s_X[GRID_X_STRIDE*%d]);" % i)
            self.gen_add_code_line("grid_xtmul_peq(F_%d, X, F_%d); grid_pin6(F_%d);" % (p, i, p))
            self.gen_add_code_line("// I^C_parent += X^T I^C X, one column per lane, transposed through LDS")
            self.gen_add_code_line("T Tc[6], Tr[6];")
            self.gen_add_code_line("grid_xtmul(Tc, X, IC_%d);" % i)
            gen_inertia_to_parent(self, i, "IC_%d" % p, use_thread_group)
        self.gen_add_end_control_flow()

    self.gen_tree_traversal(pre, post)
    self.gen_add_code_line("// publish: lane j writes M[i][j] for i <= j into both slots (every pair once: exactly symmetric; 0 where i is not an ancestor of j)")
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    for i in range(n):
        self.gen_add_code_line("if (lane >= %d) { s_M[%d + lane] = Mcol[%d]; s_M[lane*%d + %d] = Mcol[%d]; }" % (i, i * ld, i, ld, i, i))
    self.gen_add_end_control_flow()
    self.gen_add_end_function()


def gen_crba_device(self, use_thread_group=False):
    self.gen_add_func_doc("Compute the joint-space inertia matrix M(q): X(q) update + crba_inner (lane-group cooperative)",
                          ["all lanes of the solve's lane group must call it; s_M (dense, symmetric) is visible to the group on return",
                           "uses GRID_OFF_X and, by robot, GRID_OFF_U | GRID_OFF_T or off_sp of s_work (CRBA_LDS_PER_SOLVE elements suffice)"],
                          ["s_M is the n x n output in LDS (leading dimension GRID_MINV_LD)", "s_q is the vector of joint positions in LDS",
                           "s_work is this solve's LDS workspace", "d_robotModel is the pointer to the initialized model specific helpers on the GPU",
                           "lane is the caller's lane index inside the solve's lane group",
                           "off_sp is the offset of the path-axis scratch of branch-frame robots inside s_work (the kernel passes CRBA_OFF_SP)"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void crba_device(T *s_M, const T *s_q, T *s_work, const robotModel<T> *d_robotModel, const int lane, const int off_sp = GRID_OFF_SP) {", True)
    self.gen_add_code_line("T *s_X = &s_work[GRID_OFF_X]; T *s_T = &s_work[GRID_OFF_T]; (void)s_T; (void)off_sp; // (off_sp: path-axis scratch of branch-frame robots inside s_work)")
    self.gen_load_update_XImats_helpers_function_call(use_thread_group)
    self.gen_crba_inner_function_call(use_thread_group)
    self.gen_add_end_function()


def gen_crba_kernel(self, use_thread_group=False, single_call_timing=False):
    n = self.model.n
    func_params = ["d_M is the output: dense symmetric M, d_M[k*n*n + col*n + row] (both triangles, structural zeros included)",
                   "d_q_qd is the vector of joint positions (and velocities): only the first n values of every row are read",
                   "stride_q_qd is the stride between each row",
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU (XImats, topology_helpers, etc.)",
                   "gravity is accepted for the reference's signature and unused: M(q) does not depend on it",
                   "num_timesteps is the length of the trajectory points we need to compute over (or overloaded as test_iters for timing)"]
    func_def = "void crba_kernel(T *d_M, const T *d_q_qd, const int stride_q_qd, const robotModel<T> *d_robotModel, const T gravity, const int NUM_TIMESTEPS) {"
    notes = []
    if single_call_timing:
        func_def = func_def.replace("kernel(", "kernel_single_timing(")
        notes = ["one solve on the first lane group, NUM_TIMESTEPS repetitions (the input stays in LDS untouched: every repetition computes the same M)"]
    self.gen_add_func_doc("Compute the CRBA (Composite Rigid Body Algorithm)", notes, func_params, None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__global__ GRID_LAUNCH_BOUNDS")
    self.gen_add_code_line(func_def, True)
    self.gen_kernel_prologue("CRBA_LDS_PER_SOLVE")
    self.gen_add_code_lines(["(void)gravity;",
                             "T *s_q_qd = &s_mem[GRID_OFF_IN];",
                             "T *s_M = &s_mem[CRBA_OFF_M]; T *s_out = &s_out_all[grp*%d];" % (n * n)])
    if single_call_timing:
        self.gen_add_code_line("const int k = 0; const int kc = 0; const bool valid = (blockIdx.x + blockIdx.y == 0) && (grp == 0); const int lane = lane_id; (void)k;")
        self.gen_add_code_line("if (!valid) {return;}")
    else:
        self.gen_add_parallel_loop("k", "NUM_TIMESTEPS", use_thread_group, block_level=True)
    self.gen_kernel_load_inputs("q_qd", "stride_q_qd", n, use_thread_group)
    if single_call_timing:
        self.gen_add_code_line("for (int rep = 0; rep < NUM_TIMESTEPS; rep++){", True)
    self.gen_add_code_line("// compute")
    if single_call_timing:
        self.gen_add_code_line("const int lane_r = grid_loop_variant(lane_id); // (keeps lane-dependent values from being hoisted out of the repetition loop and spilled)")
        self.gen_add_code_line("crba_device<T>(s_M, s_q_qd, s_mem, d_robotModel, lane_r, CRBA_OFF_SP);")
        self.gen_add_end_control_flow()
    else:
        self.gen_add_code_line("crba_device<T>(s_M, s_q_qd, s_mem, d_robotModel, lane, CRBA_OFF_SP);")
    self.gen_add_code_line("// dense record (leading dimension n) in the staging area")
    self.gen_add_parallel_loop("ind", str(n * n), use_thread_group)
    self.gen_add_code_line("const int row = ind %% %d; const int col = ind / %d;" % (n, n))
    self.gen_add_code_line("s_out[ind] = s_M[col*%d + row];" % self.minv_ld)
    self.gen_add_end_control_flow()
    if single_call_timing:
        self.gen_kernel_save_result_single_timing("M", n * n, use_thread_group, "s_out")
    else:
        self.gen_kernel_save_result("M", n * n, n * n, use_thread_group, "s_out")
        self.gen_add_end_control_flow()
    self.gen_add_end_function()


def gen_crba_host(self, mode=0):
    single_call_timing = mode == 1
    compute_only = mode == 2
    func_params = ["hd_data is the packaged input and output pointers (d_M / h_M are allocated by the first call and grown by longer ones)",
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU (XImats, topology_helpers, etc.)",
                   "gravity is accepted for the reference's signature and unused",
                   "num_timesteps is the length of the trajectory points we need to compute over (or overloaded as test_iters for timing)",
                   "streams are pointers to HIP streams for async memory transfers (if needed)"]
    name = "crba" + ("_single_timing" if single_call_timing else "") + ("_compute_only" if compute_only else "")
    notes = ["USE_COMPRESSED_MEM: rows of d_q_qd / h_q_qd (stride 2n), otherwise of d_q_qd_u / h_q_qd_u (stride 3n); the first n values of a row are q",
             "_single_timing: one solve repeated num_timesteps times in one launch, time per repetition printed; h_M holds that solve's M"] if mode == 0 else []
    self.gen_add_func_doc("Compute the CRBA (Composite Rigid Body Algorithm)", notes, func_params, None)
    self.gen_add_code_line("template <typename T, bool USE_COMPRESSED_MEM = false>")
    self.gen_add_code_line("__host__")
    self.gen_add_code_line("void " + name + "(gridData<T> *hd_data, const robotModel<T> *d_robotModel, const T gravity, const int num_timesteps,")
    self.gen_add_code_line("                      const dim3 block_dimms, const dim3 thread_dimms" + ("" if compute_only else ", hipStream_t *streams") + ") {", True)
    cnt = "1" if single_call_timing else "num_timesteps"
    self.gen_add_code_lines(["grid_ee_reserve<T>(&hd_data->d_M, &hd_data->h_M, NUM_JOINTS*NUM_JOINTS, %s);" % cnt,
                             "const int stride_q_qd = USE_COMPRESSED_MEM ? 2*NUM_JOINTS : 3*NUM_JOINTS;",
                             "T *d_in = USE_COMPRESSED_MEM ? hd_data->d_q_qd : hd_data->d_q_qd_u;"])
    if not compute_only:
        self.gen_add_code_lines(["// start code with memory transfer",
                                 "gpuErrchk(hipMemcpyAsync(d_in, USE_COMPRESSED_MEM ? hd_data->h_q_qd : hd_data->h_q_qd_u, static_cast<size_t>(stride_q_qd)*" + cnt + "*sizeof(T), hipMemcpyHostToDevice, streams[0]));",
                                 "gpuErrchk(hipDeviceSynchronize());"])
    kern = "crba_kernel" + ("_single_timing" if single_call_timing else "") + "<T>"
    self.gen_add_code_line("// then call the kernel")
    if single_call_timing:
        self.gen_add_code_line("struct timespec start, end; clock_gettime(CLOCK_MONOTONIC,&start);")
    self.gen_add_code_lines(["hipLaunchKernelGGL((" + kern + "),block_dimms,thread_dimms,grid_lds_bytes<T>(thread_dimms, CRBA_LDS_PER_SOLVE, CRBA_OUT_PER_SOLVE),0,hd_data->d_M,d_in,stride_q_qd,d_robotModel,gravity,num_timesteps);",
                             "gpuErrchk(hipGetLastError()); gpuErrchk(hipDeviceSynchronize());"])
    if single_call_timing:
        self.gen_add_code_line("clock_gettime(CLOCK_MONOTONIC,&end);")
    if not compute_only:
        self.gen_add_code_lines(["// finally transfer the result back",
                                 "gpuErrchk(hipMemcpy(hd_data->h_M,hd_data->d_M,static_cast<size_t>(NUM_JOINTS*NUM_JOINTS)*" + cnt + "*sizeof(T),hipMemcpyDeviceToHost));",
                                 "gpuErrchk(hipDeviceSynchronize());"])
    if single_call_timing:
        self.gen_add_code_line("printf(\"Single Call CRBA %fus\\n\",time_delta_us_timespec(start,end)/static_cast<double>(num_timesteps));")
    self.gen_add_end_function()


def gen_crba_constants(self):
    K = self.gen_lds_layout()["KERNELS"]["CRBA"]
    self.gen_add_code_line("//")
    self.gen_add_code_line("// crba: joint-space inertia matrix M(q), %s.  Slice: %s" % (
        {"tip": "tip-frame form (crba_inner_tip)", "branch": "branch-frame form (crba_inner_branch)", "walk": "column walk (crba_inner)"}[crba_form(self)],
        "the compact slice of direct_minv (IN | X | path axes | M)" if K["compact"] else "IN | X | U | T of the general slice, M where the general slice keeps M^-1"))
    self.gen_add_code_line("//")
    self.gen_add_code_lines(["const int CRBA_LDS_PER_SOLVE = %d; const int CRBA_OUT_PER_SOLVE = %d; const int CRBA_OFF_M = %d; const int CRBA_OFF_SP = %d; const int CRBA_SUGGESTED_THREADS = %s;"
                             % (K["LDS"], K["OUT"], K["MINV"], K["SP"], "64" if K["compact"] else "SUGGESTED_THREADS"),
                             "const int CRBA_DYNAMIC_SHARED_MEM_COUNT = GRID_MAX_SOLVES_PER_BLOCK*(CRBA_LDS_PER_SOLVE + CRBA_OUT_PER_SOLVE);",
                             "const int CRBA_SHARED_MEM_COUNT = CRBA_DYNAMIC_SHARED_MEM_COUNT; // (the reference's name: elements of T for SUGGESTED_THREADS threads)"])


def gen_crba(self, use_thread_group=False):
    self.gen_crba_constants()
    self.gen_crba_inner(use_thread_group)
    self.gen_crba_device(use_thread_group)
    self.gen_crba_kernel(use_thread_group, True)
    self.gen_crba_kernel(use_thread_group, False)
    for mode in (0, 1, 2):
        self.gen_crba_host(mode)
