"""End-effector kinematics: pose, its gradient and its Hessian, emitter for the HIP/CDNA4 backend.

Mirrors the role of the reference's algorithms/_eepose_gradient_hessian.py (end_effector_pose :1-200, gradient :400-560, Hessian :900-1060,
gen_eepose_and_derivatives): for every leaf joint e of the tree (ascending id) the base-frame transform T_e(q) = T_root(q_root) ... T_leaf(q_leaf)
with T_j(q) = [R_tree_j Rot(axis_j, q) | xyz_j] (revolute) or [R_tree_j | xyz_j + R_tree_j axis_j q] (prismatic), and the 6-vector
[x, y, z, roll, pitch, yaw] with roll = atan2(R21, R22), pitch = -atan2(R20, sqrt(R21^2 + R22^2)), yaw = atan2(R10, R00) (reference :155-157).
No tool offset (the reference's own "TODO: ADD OFFSETS" stands).

Layouts (k = batch index, array-of-structs over k):
    eePos   [k*6E + 6e + c]
    deePos  [k*6En + 6(e*n + j) + c]                      (reference :517-521)
    d2eePos [k*6En^2 + e*6n^2 + c*n^2 + i*n + j]          (reference :1003-1024 for E = 1.  For E > 1 the reference writes every end effector into
                                                           the same 6n^2 slots - its offsets ignore curr_ee - which is a defect; here e has its own block)

Lane-group form (lane j <-> joint j):
  1. lane j builds its joint's local transform from q_j (grid_sincos) and its joint axis in the parent frame (LDS, 16 values per joint);
  2. lane j composes its root path (parents' local transforms, read from LDS): base-frame R_j, p_j and the base-frame joint axis w_j;
  3. gradient: lane j owns column j of every leaf below it: revolute d(p, R) = (w_j x (p_e - p_j), [w_j]x R_e), prismatic (w_j, 0); the angle rows
     follow from the five R entries the atan2 formulas use;
  4. Hessian: lane j owns column j; for i on the same root path the ancestor a = min(i, j) and the descendant d = max(i, j) give
     d2(p, R) = revolute(a) ? w_a x d(p, R)/dq_d : 0.  Both (i, j) and (j, i) evaluate the same call with the same (a, d): the record is exactly symmetric.
Records that fit (pose, gradient, Hessians of <= EE_STAGE_MAX values) are staged in LDS and leave wave-cooperatively in 16-byte pieces
(gen_kernel_save_result); larger Hessians are stored straight from the lanes, one contiguous run of n values per (e, c, i) and solve.
"""
import numpy as np

EE_STAGE_MAX = 1024  # Hessian records up to this many values per solve are staged in LDS


def _ee_leaves(self):
    m = self.model
    return [j for j in range(m.n) if not m.children[j]]


def _ee_path_mask(self, leaf):
    m = self.model
    mask = 1 << leaf
    for a in m.ancestors[leaf]:
        mask |= 1 << a
    return mask


def _ee_hess_staged(self):
    n, E = self.model.n, len(_ee_leaves(self))
    return 6 * E * n * n <= EE_STAGE_MAX


def _ee_joint_constants(self):
    """16 values per joint: R_tree (row-major, child -> parent), xyz, the joint axis in the parent frame (R_tree e_axis), 1 = revolute / 0 = prismatic.
    Recovered from X_tree = [[R^T, 0], [-R^T skew(xyz), R^T]]."""
    m = self.model
    vals = []
    for j in range(m.n):
        XT = m.X_tree[j]
        R = XT[:3, :3].T
        S = -R @ XT[3:, :3]
        xyz = [S[2, 1], S[0, 2], S[1, 0]]
        s = m.S_index[j]
        u = R[:, s % 3]
        vals += [R[r, c] for r in range(3) for c in range(3)] + list(xyz) + list(u) + [1.0 if s < 3 else 0.0]
    return [0.0 if abs(v) < 1e-15 else float(v) for v in vals]


def _ee_lds(self):
    """per-solve slice of the kinematics kernels: q (padded) | local transforms (16 n) | base-frame transforms (16 n)"""
    n = self.model.n
    off_in = 0
    off_l = (n + 3) // 4 * 4
    off_w = off_l + 16 * n
    return dict(IN=off_in, L=off_l, W=off_w, TOTAL=off_w + 16 * n)


def gen_end_effector_pose_inner_temp_mem_size(self):
    return _ee_lds(self)["TOTAL"]


def gen_end_effector_pose_gradient_inner_temp_mem_size(self):
    return _ee_lds(self)["TOTAL"]


def gen_end_effector_pose_gradient_hessian_inner_temp_mem_size(self):
    return _ee_lds(self)["TOTAL"]


def _ee_out_sizes(self):
    n, E = self.model.n, len(_ee_leaves(self))
    return 6 * E, 6 * E * n, 6 * E * n * n


def gen_eepose_constants(self):
    """constants, tables and the shared device helpers of the kinematics kernels"""
    m = self.model
    n = m.n
    leaves = _ee_leaves(self)
    E = len(leaves)
    lds = _ee_lds(self)
    pos, grad, hess = _ee_out_sizes(self)
    staged = _ee_hess_staged(self)
    self.gen_add_code_line("//")
    self.gen_add_code_line("// end-effector kinematics (end_effector_pose / _gradient / _gradient_hessian): every leaf joint is an end effector (ascending id)")
    self.gen_add_code_line("//")
    self.gen_add_code_lines(["const int EE_OFF_IN = %d; const int EE_OFF_L = %d; const int EE_OFF_W = %d; // slice: q | local transforms | base-frame transforms (16 values per joint)" % (lds["IN"], lds["L"], lds["W"]),
                             "const int EE_POS_LDS_PER_SOLVE = %d; const int EE_POS_OUT_PER_SOLVE = %d; const int EE_POS_SUGGESTED_THREADS = SUGGESTED_THREADS;" % (lds["TOTAL"], pos),
                             "const int DEE_POS_LDS_PER_SOLVE = %d; const int DEE_POS_OUT_PER_SOLVE = %d; const int DEE_POS_SUGGESTED_THREADS = SUGGESTED_THREADS;" % (lds["TOTAL"], grad),
                             "const int D2EE_POS_LDS_PER_SOLVE = %d; const int D2EE_POS_OUT_PER_SOLVE = %d; const int D2EE_POS_SUGGESTED_THREADS = SUGGESTED_THREADS;%s"
                             % (lds["TOTAL"], grad + (hess if staged else 0), " // gradient + Hessian staging" if staged else " // gradient staging; the Hessian (%d values per solve) is stored straight from the lanes" % hess),
                             "#define GRID_EE_HESS_STAGED %d // 1: the Hessian record of a solve is staged in LDS" % (1 if staged else 0),
                             "const int EE_POS_DYNAMIC_SHARED_MEM_COUNT = GRID_MAX_SOLVES_PER_BLOCK*(EE_POS_LDS_PER_SOLVE + EE_POS_OUT_PER_SOLVE);",
                             "const int DEE_POS_DYNAMIC_SHARED_MEM_COUNT = GRID_MAX_SOLVES_PER_BLOCK*(DEE_POS_LDS_PER_SOLVE + DEE_POS_OUT_PER_SOLVE);",
                             "const int D2EE_POS_DYNAMIC_SHARED_MEM_COUNT = GRID_MAX_SOLVES_PER_BLOCK*(D2EE_POS_LDS_PER_SOLVE + D2EE_POS_OUT_PER_SOLVE);"])
    self.gen_add_code_line("// leaf joints (end effectors), root path of every leaf as a joint bit mask, parent of every joint")
    self.gen_add_code_line("__device__ const int grid_ee_leaves[%d] = {%s};" % (E, ", ".join(str(x) for x in leaves)))
    self.gen_add_code_line("const int GRID_EE_JOINTS[%d] = {%s}; // (host copy of grid_ee_leaves)" % (E, ", ".join(str(x) for x in leaves)))
    self.gen_add_code_line("__device__ const unsigned long long grid_ee_path[%d] = {%s};" % (E, ", ".join("0x%xull" % _ee_path_mask(self, l) for l in leaves)))
    self.gen_add_code_line("__device__ const int grid_ee_parent[%d] = {%s};" % (n, ", ".join(str(int(p)) for p in m.parent)))
    vals = _ee_joint_constants(self)
    self.gen_add_code_line("// per joint: R_tree (row-major), xyz, joint axis in the parent frame, 1 = revolute / 0 = prismatic")
    for ctype, sfx in (("float", "f"), ("double", "")):
        self.gen_add_code_line("__device__ const %s grid_ee_constants_%s[%d] = {" % (ctype, ctype, len(vals)), True)
        for k in range(0, len(vals), 8):
            self.gen_add_code_line(", ".join(repr(float(v)) + sfx for v in vals[k:k + 8]) + ("," if k + 8 < len(vals) else ""))
        self.indent_level -= 1
        self.gen_add_code_line("};")
    self.gen_add_code_lines([
        "__device__ __forceinline__ const float *grid_ee_constants(const float *) { return grid_ee_constants_float; }",
        "__device__ __forceinline__ const double *grid_ee_constants(const double *) { return grid_ee_constants_double; }",
        "// first derivative of a leaf's (p, R) with respect to joint j (base-frame record Wj: R row-major | origin | axis | revolute flag):",
        "// g[0..2] = dp, g[3 + 3r + c] = dR[r][c];  revolute: (w x (p_e - p_j), [w]x R_e), prismatic: (w, 0)",
        "template <typename T>",
        "__device__ __forceinline__ void grid_ee_d1(T (&g)[12], const T *Wj, const T (&Re)[9], const T (&pe)[3]) {",
        "    const T wx = Wj[12], wy = Wj[13], wz = Wj[14];",
        "    const bool rev = Wj[15] != static_cast<T>(0);",
        "    const T rx = pe[0] - Wj[9], ry = pe[1] - Wj[10], rz = pe[2] - Wj[11];",
        "    g[0] = rev ? wy*rz - wz*ry : wx;",
        "    g[1] = rev ? wz*rx - wx*rz : wy;",
        "    g[2] = rev ? wx*ry - wy*rx : wz;",
        "    #pragma unroll",
        "    for (int c = 0; c < 3; c++) {",
        "        g[3 + c] = rev ? wy*Re[6 + c] - wz*Re[3 + c] : static_cast<T>(0);",
        "        g[6 + c] = rev ? wz*Re[c] - wx*Re[6 + c] : static_cast<T>(0);",
        "        g[9 + c] = rev ? wx*Re[3 + c] - wy*Re[c] : static_cast<T>(0);",
        "    }",
        "}",
        "// roll, pitch, yaw of a rotation (reference _eepose_gradient_hessian.py:155-157)",
        "template <typename T>",
        "__device__ __forceinline__ void grid_ee_rpy(T *out, const T (&R)[9]) {",
        "    out[0] = atan2(R[7], R[8]);",
        "    out[1] = -atan2(R[6], sqrt(R[7]*R[7] + R[8]*R[8]));",
        "    out[2] = atan2(R[3], R[0]);",
        "}",
        "// first derivatives of roll, pitch, yaw from dR (g as grid_ee_d1)",
        "template <typename T>",
        "__device__ __forceinline__ void grid_ee_rpy_d1(T *out, const T (&R)[9], const T (&g)[12]) {",
        "    const T D0 = R[7]*R[7] + R[8]*R[8];",
        "    const T s = sqrt(D0);",
        "    const T ds = (R[7]*g[10] + R[8]*g[11])/s;",
        "    out[0] = (R[8]*g[10] - R[7]*g[11])/D0;",
        "    out[1] = -(s*g[9] - R[6]*ds)/(R[6]*R[6] + D0);",
        "    out[2] = (R[0]*g[6] - R[3]*g[3])/(R[0]*R[0] + R[3]*R[3]);",
        "}",
        "// d2 atan2(y, x)/dq_i dq_j from the values, both first derivatives and the second derivative of x and y",
        "template <typename T>",
        "__device__ __forceinline__ T grid_ee_atan2_d2(const T x, const T y, const T xi, const T yi, const T xj, const T yj, const T xij, const T yij) {",
        "    const T D = x*x + y*y;",
        "    const T Nj = x*yj - y*xj;",
        "    const T dNj = xi*yj + x*yij - yi*xj - y*xij;",
        "    const T dD = static_cast<T>(2)*(x*xi + y*yi);",
        "    return (dNj*D - Nj*dD)/(D*D);",
        "}",
        "// d2 pose/dq_a dq_d for an ancestor a (or a == d) and a descendant d on one leaf's root path: d2(p, R) = revolute(a) ? w_a x d(p, R)/dq_d : 0",
        "template <typename T>",
        "__device__ __forceinline__ void grid_ee_d2(T *v, const T *Wa, const T *Wd, const T (&Re)[9], const T (&pe)[3]) {",
        "    T ga[12], gd[12], h[12];",
        "    grid_ee_d1(ga, Wa, Re, pe);",
        "    grid_ee_d1(gd, Wd, Re, pe);",
        "    const T wx = Wa[12], wy = Wa[13], wz = Wa[14];",
        "    const bool rev = Wa[15] != static_cast<T>(0);",
        "    #pragma unroll",
        "    for (int b = 0; b < 12; b += 3) {",
        "        const int i0 = b == 0 ? 0 : 3 + (b - 3)/3, st = b == 0 ? 1 : 3; // (p, then the columns of R)",
        "        const T x = gd[i0], y = gd[i0 + st], z = gd[i0 + 2*st];",
        "        h[i0] = rev ? wy*z - wz*y : static_cast<T>(0);",
        "        h[i0 + st] = rev ? wz*x - wx*z : static_cast<T>(0);",
        "        h[i0 + 2*st] = rev ? wx*y - wy*x : static_cast<T>(0);",
        "    }",
        "    v[0] = h[0]; v[1] = h[1]; v[2] = h[2];",
        "    v[3] = grid_ee_atan2_d2(Re[8], Re[7], ga[11], ga[10], gd[11], gd[10], h[11], h[10]);",
        "    const T s = sqrt(Re[7]*Re[7] + Re[8]*Re[8]);",
        "    const T si = (Re[7]*ga[10] + Re[8]*ga[11])/s, sj = (Re[7]*gd[10] + Re[8]*gd[11])/s;",
        "    const T sij = (ga[10]*gd[10] + Re[7]*h[10] + ga[11]*gd[11] + Re[8]*h[11] - si*sj)/s;",
        "    v[4] = -grid_ee_atan2_d2(s, Re[6], si, ga[9], sj, gd[9], sij, h[9]);",
        "    v[5] = grid_ee_atan2_d2(Re[0], Re[3], ga[3], ga[6], gd[3], gd[6], h[3], h[6]);",
        "}",
        "template <typename T>",
        "__device__ __forceinline__ void grid_ee_load_frame(T (&R)[9], T (&p)[3], const T *W) {",
        "    #pragma unroll",
        "    for (int r = 0; r < 9; r++) { R[r] = W[r]; }",
        "    p[0] = W[9]; p[1] = W[10]; p[2] = W[11];",
        "}", ""])


def gen_end_effector_pose_inner(self, use_thread_group=False):
    m = self.model
    n = m.n
    self.gen_add_func_doc("Base-frame transforms of every joint of one solve (the kinematics all three end-effector algorithms start from)",
                          ["lane j builds T_j(q_j) into s_L, then composes its root path into s_W[16 j]: R (row-major), origin, joint axis, revolute flag",
                           "all lanes of the lane group must call it; s_W is visible to the group on return"],
                          ["s_W is the base-frame transform storage (16 values per joint)", "s_L is the local transform storage (16 values per joint)",
                           "s_q is the vector of joint positions", "lane is the caller's lane index inside the solve's lane group"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void end_effector_pose_inner(T *s_W, T *s_L, const T *s_q, const int lane) {", True)
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_lines(["const T *C = &grid_ee_constants(static_cast<const T *>(nullptr))[16*lane];",
                             "T *L = &s_L[16*lane];",
                             "const T q = s_q[lane];"])
    types = sorted(set(m.S_index))
    if any(s_ < 3 for s_ in types):
        self.gen_add_code_line("T sn, cs; grid_sincos(q, &sn, &cs);")
    first = True
    for s in types:
        ids = [j for j in range(n) if m.S_index[j] == s]
        cond = "" if len(types) == 1 else (("if " if first else "else if ") + self.gen_lane_mask_test(ids) + " ")
        first = False
        a = s % 3
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        self.gen_add_code_line(cond + "{ // " + ("revolute" if s < 3 else "prismatic") + " about " + "xyz"[a] + ": joints " + str(ids), True)
        self.gen_add_code_line("#pragma unroll")
        self.gen_add_code_line("for (int r = 0; r < 3; r++) {", True)
        if s < 3:  # R_tree Rot(a, q): column a kept, columns a1, a2 rotate
            self.gen_add_code_line("L[3*r+%d] = C[3*r+%d];" % (a, a))
            self.gen_add_code_line("L[3*r+%d] = cs*C[3*r+%d] + sn*C[3*r+%d];" % (a1, a1, a2))
            self.gen_add_code_line("L[3*r+%d] = cs*C[3*r+%d] - sn*C[3*r+%d];" % (a2, a2, a1))
            self.gen_add_code_line("L[9+r] = C[9+r];")
        else:  # translation along the axis
            self.gen_add_code_line("L[3*r] = C[3*r]; L[3*r+1] = C[3*r+1]; L[3*r+2] = C[3*r+2];")
            self.gen_add_code_line("L[9+r] = C[9+r] + q*C[3*r+%d];" % a)
        self.gen_add_end_control_flow()
        self.gen_add_end_control_flow()
    self.gen_add_code_line("L[12] = C[12]; L[13] = C[13]; L[14] = C[14]; L[15] = C[15];")
    self.gen_add_end_control_flow()
    self.gen_add_sync(use_thread_group)
    self.gen_add_code_line("// compose the root path: T_j <- T_parent T_j, axis <- R_parent axis")
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_lines(["T R[9], p[3], w[3];",
                             "const T *Lj = &s_L[16*lane];",
                             "grid_ee_load_frame(R, p, Lj);",
                             "w[0] = Lj[12]; w[1] = Lj[13]; w[2] = Lj[14];",
                             "for (int a = grid_ee_parent[lane]; a >= 0; a = grid_ee_parent[a]) {"])
    self.indent_level += 1
    self.gen_add_code_lines(["T Ra[9], pa[3], t[9], tp[3], tw[3];",
                             "grid_ee_load_frame(Ra, pa, &s_L[16*a]);",
                             "#pragma unroll",
                             "for (int r = 0; r < 3; r++) {",
                             "    #pragma unroll",
                             "    for (int c = 0; c < 3; c++) { t[3*r+c] = Ra[3*r]*R[c] + Ra[3*r+1]*R[3+c] + Ra[3*r+2]*R[6+c]; }",
                             "    tp[r] = Ra[3*r]*p[0] + Ra[3*r+1]*p[1] + Ra[3*r+2]*p[2] + pa[r];",
                             "    tw[r] = Ra[3*r]*w[0] + Ra[3*r+1]*w[1] + Ra[3*r+2]*w[2];",
                             "}",
                             "#pragma unroll",
                             "for (int r = 0; r < 9; r++) { R[r] = t[r]; }",
                             "#pragma unroll",
                             "for (int r = 0; r < 3; r++) { p[r] = tp[r]; w[r] = tw[r]; }"])
    self.gen_add_end_control_flow()
    self.gen_add_code_lines(["T *Wj = &s_W[16*lane];",
                             "#pragma unroll",
                             "for (int r = 0; r < 9; r++) { Wj[r] = R[r]; }",
                             "Wj[9] = p[0]; Wj[10] = p[1]; Wj[11] = p[2]; Wj[12] = w[0]; Wj[13] = w[1]; Wj[14] = w[2]; Wj[15] = Lj[15];"])
    self.gen_add_end_control_flow()
    self.gen_add_sync(use_thread_group)
    self.gen_add_end_function()


def gen_end_effector_pose_device(self, use_thread_group=False):
    E = len(_ee_leaves(self))
    self.gen_add_func_doc("Compute the end-effector poses [x, y, z, roll, pitch, yaw] of one solve",
                          ["lanes 0..NUM_EES-1 write s_eePos[6e + c]; the caller must grid_wave_sync() before other lanes read it"],
                          ["s_eePos is the output record (6 NUM_EES values)", "s_q is the vector of joint positions",
                           "s_work is this solve's LDS workspace of EE_POS_LDS_PER_SOLVE elements",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU (unused: the kinematics constants are baked in)",
                           "lane is the caller's lane index inside the solve's lane group"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void end_effector_pose_device(T *s_eePos, const T *s_q, T *s_work, const robotModel<T> *d_robotModel, const int lane) {", True)
    self.gen_add_code_line("(void)d_robotModel;")
    self.gen_add_code_line("end_effector_pose_inner<T>(&s_work[EE_OFF_W], &s_work[EE_OFF_L], s_q, lane);")
    self.gen_add_code_line("if (lane < %d) {" % E, True)
    self.gen_add_code_lines(["T R[9], p[3]; grid_ee_load_frame(R, p, &s_work[EE_OFF_W + 16*grid_ee_leaves[lane]]);",
                             "T *o = &s_eePos[6*lane];",
                             "o[0] = p[0]; o[1] = p[1]; o[2] = p[2];",
                             "grid_ee_rpy(&o[3], R);"])
    self.gen_add_end_control_flow()
    self.gen_add_end_function()


def gen_end_effector_pose_gradient_inner(self, use_thread_group=False):
    n = self.model.n
    E = len(_ee_leaves(self))
    self.gen_add_func_doc("Gradient of the end-effector poses from the base-frame transforms",
                          ["lane j writes column j of every end effector: s_deePos[6(e n + j) + c] (0 where joint j is not on the leaf's root path)"],
                          ["s_deePos is the output record (6 NUM_EES NUM_JOINTS values)", "s_W holds the base-frame transforms (end_effector_pose_inner)",
                           "lane is the caller's lane index inside the solve's lane group"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void end_effector_pose_gradient_inner(T *s_deePos, const T *s_W, const int lane) {", True)
    self.gen_add_code_line("if (lane < %d) {" % n, True)
    self.gen_add_code_line("for (int e = 0; e < %d; e++) {" % E, True)
    self.gen_add_code_lines(["T Re[9], pe[3]; grid_ee_load_frame(Re, pe, &s_W[16*grid_ee_leaves[e]]);",
                             "T o[6] = {static_cast<T>(0), static_cast<T>(0), static_cast<T>(0), static_cast<T>(0), static_cast<T>(0), static_cast<T>(0)};",
                             "if ((grid_ee_path[e] >> lane) & 1ull) {",
                             "    T g[12]; grid_ee_d1(g, &s_W[16*lane], Re, pe);",
                             "    o[0] = g[0]; o[1] = g[1]; o[2] = g[2];",
                             "    grid_ee_rpy_d1(&o[3], Re, g);",
                             "}",
                             "#pragma unroll",
                             "for (int c = 0; c < 6; c++) { s_deePos[6*(e*%d + lane) + c] = o[c]; }" % n])
    self.gen_add_end_control_flow()
    self.gen_add_end_control_flow()
    self.gen_add_end_function()


def gen_end_effector_pose_gradient_device(self, use_thread_group=False):
    self.gen_add_func_doc("Compute the gradient of the end-effector poses of one solve",
                          ["all lanes of the solve's lane group must call it; the caller must grid_wave_sync() before other lanes read s_deePos"],
                          ["s_deePos is the output record (6 NUM_EES NUM_JOINTS values)", "s_q is the vector of joint positions",
                           "s_work is this solve's LDS workspace of DEE_POS_LDS_PER_SOLVE elements",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU (unused)",
                           "lane is the caller's lane index inside the solve's lane group"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void end_effector_pose_gradient_device(T *s_deePos, const T *s_q, T *s_work, const robotModel<T> *d_robotModel, const int lane) {", True)
    self.gen_add_code_line("(void)d_robotModel;")
    self.gen_add_code_line("end_effector_pose_inner<T>(&s_work[EE_OFF_W], &s_work[EE_OFF_L], s_q, lane);")
    self.gen_add_code_line("end_effector_pose_gradient_inner<T>(s_deePos, &s_work[EE_OFF_W], lane);")
    self.gen_add_end_function()


def gen_end_effector_pose_gradient_hessian_inner(self, use_thread_group=False):
    n = self.model.n
    E = len(_ee_leaves(self))
    self.gen_add_func_doc("Hessian of the end-effector poses from the base-frame transforms",
                          ["lane j writes column j: d2eePos[e 6n^2 + c n^2 + i n + j] for every e, c, i (0 unless both joints are on the leaf's root path);",
                           "(i, j) and (j, i) are one call with (ancestor, descendant) = (min, max): the record is exactly symmetric"],
                          ["d2 is this solve's output record (LDS staging or global memory)", "s_W holds the base-frame transforms (end_effector_pose_inner)",
                           "lane is the caller's lane index inside the solve's lane group", "active is false for lane groups past the end of the batch (nothing is written)"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void end_effector_pose_gradient_hessian_inner(T *d2, const T *s_W, const int lane, const bool active) {", True)
    self.gen_add_code_line("if (active && lane < %d) {" % n, True)
    self.gen_add_code_line("for (int e = 0; e < %d; e++) {" % E, True)
    self.gen_add_code_lines(["T Re[9], pe[3]; grid_ee_load_frame(Re, pe, &s_W[16*grid_ee_leaves[e]]);",
                             "const unsigned long long path = grid_ee_path[e];",
                             "const bool onj = (path >> lane) & 1ull;",
                             "T *dst = &d2[e*%d + lane];" % (6 * n * n),
                             "for (int i = 0; i < %d; i++) {" % n])
    self.indent_level += 1
    self.gen_add_code_lines(["T v[6] = {static_cast<T>(0), static_cast<T>(0), static_cast<T>(0), static_cast<T>(0), static_cast<T>(0), static_cast<T>(0)};",
                             "if (onj && ((path >> i) & 1ull)) {",
                             "    const int a = i < lane ? i : lane, d = i < lane ? lane : i;",
                             "    grid_ee_d2(v, &s_W[16*a], &s_W[16*d], Re, pe);",
                             "}",
                             "#pragma unroll",
                             "for (int c = 0; c < 6; c++) { dst[c*%d + i*%d] = v[c]; }" % (n * n, n)])
    self.gen_add_end_control_flow()
    self.gen_add_end_control_flow()
    self.gen_add_end_control_flow()
    self.gen_add_end_function()


def gen_end_effector_pose_gradient_hessian_device(self, use_thread_group=False):
    self.gen_add_func_doc("Compute the gradient and the Hessian of the end-effector poses of one solve",
                          ["all lanes of the solve's lane group must call it; the caller must grid_wave_sync() before other lanes read s_deePos or a staged d2"],
                          ["d2 is this solve's Hessian record (6 NUM_EES NUM_JOINTS^2 values: LDS staging or global memory)",
                           "s_deePos is the gradient record (6 NUM_EES NUM_JOINTS values)", "s_q is the vector of joint positions",
                           "s_work is this solve's LDS workspace of D2EE_POS_LDS_PER_SOLVE elements",
                           "d_robotModel is the pointer to the initialized model specific helpers on the GPU (unused)",
                           "lane is the caller's lane index inside the solve's lane group", "active is false for lane groups past the end of the batch"], None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__device__ __forceinline__")
    self.gen_add_code_line("void end_effector_pose_gradient_hessian_device(T *d2, T *s_deePos, const T *s_q, T *s_work, const robotModel<T> *d_robotModel, const int lane, const bool active) {", True)
    self.gen_add_code_line("(void)d_robotModel;")
    self.gen_add_code_line("end_effector_pose_inner<T>(&s_work[EE_OFF_W], &s_work[EE_OFF_L], s_q, lane);")
    self.gen_add_code_line("end_effector_pose_gradient_inner<T>(s_deePos, &s_work[EE_OFF_W], lane);")
    self.gen_add_code_line("grid_wave_sync(); // (the Hessian re-reads the frames after the fence: its first derivatives are not merged with the gradient's, which stays bit-identical to end_effector_pose_gradient_kernel)")
    self.gen_add_code_line("end_effector_pose_gradient_hessian_inner<T>(d2, &s_work[EE_OFF_W], lane, active);")
    self.gen_add_end_function()


_EE_KINDS = {0: ("end_effector_pose", "EE_POS"), 1: ("end_effector_pose_gradient", "DEE_POS"), 2: ("end_effector_pose_gradient_hessian", "D2EE_POS")}


def _ee_kernel(self, kind, use_thread_group=False):
    n = self.model.n
    pos, grad, hess = _ee_out_sizes(self)
    staged = _ee_hess_staged(self)
    name, C = _EE_KINDS[kind]
    params = ["d_q is the vector of joint positions", "stride_q is the stride between the q of consecutive solves (n: USE_COMPRESSED_MEM, 3n: q_qd_u)",
              "d_robotModel is the pointer to the initialized model specific helpers on the GPU (unused: the kinematics constants are baked in)",
              "NUM_TIMESTEPS is the length of the trajectory points we need to compute over"]
    if kind == 0:
        params = ["d_eePos is the output: 6 values [x, y, z, roll, pitch, yaw] per end effector, d_eePos[k*6E + 6e + c]"] + params
        sig = "T *d_eePos"
        notes = []
    elif kind == 1:
        params = ["d_deePos is the output: d_deePos[k*6En + 6(e n + j) + c]"] + params
        sig = "T *d_deePos"
        notes = []
    else:
        params = ["d_d2eePos is the output: d_d2eePos[k*6En^2 + e*6n^2 + c*n^2 + i*n + j] (the reference's layout for one end effector; for several, every",
                  "end effector has its own 6n^2 block - the reference's offsets ignore curr_ee and overlap them)",
                  "d_deePos receives the gradient as end_effector_pose_gradient_kernel writes it, or is nullptr"] + params
        sig = "T *d_d2eePos, T *d_deePos"
        notes = ["the Hessian record is " + ("staged in LDS" if staged else "stored straight from the lanes (%d values per solve do not fit LDS)" % hess)]
    self.gen_add_func_doc("Compute " + name.replace("_", " "), notes, params, None)
    self.gen_add_code_line("template <typename T>")
    self.gen_add_code_line("__global__ GRID_LAUNCH_BOUNDS")
    self.gen_add_code_line("void %s_kernel(%s, const T *d_q, const int stride_q, const robotModel<T> *d_robotModel, const int NUM_TIMESTEPS) {" % (name, sig), True)
    self.gen_kernel_prologue(C + "_LDS_PER_SOLVE")
    self.gen_add_code_line("T *s_q = &s_mem[EE_OFF_IN];")
    if kind == 0:
        self.gen_add_code_line("T *s_eePos = &s_out_all[grp*%d];" % pos)
    else:
        self.gen_add_code_line("T *s_deePos = &s_out_all[grp*%d];" % grad)
    if kind == 2 and staged:
        self.gen_add_code_line("T *s_d2eePos = &s_out_all[gpb*%d + grp*%d];" % (grad, hess))
    self.gen_add_parallel_loop("k", "NUM_TIMESTEPS", use_thread_group, block_level=True)
    self.gen_kernel_load_inputs("q", "stride_q", n, use_thread_group)
    self.gen_add_code_line("// compute")
    if kind == 0:
        self.gen_add_code_line("end_effector_pose_device<T>(s_eePos, s_q, s_mem, d_robotModel, lane);")
        self.gen_kernel_save_result("eePos", pos, pos, use_thread_group)
    elif kind == 1:
        self.gen_add_code_line("end_effector_pose_gradient_device<T>(s_deePos, s_q, s_mem, d_robotModel, lane);")
        self.gen_kernel_save_result("deePos", grad, grad, use_thread_group)
    else:
        d2 = "s_d2eePos" if staged else "&d_d2eePos[static_cast<size_t>(kc)*%d]" % hess
        self.gen_add_code_line("end_effector_pose_gradient_hessian_device<T>(%s, s_deePos, s_q, s_mem, d_robotModel, lane, valid);" % d2)
        self.gen_add_code_line("if (d_deePos != nullptr) {", True)
        self.gen_kernel_save_result("deePos", grad, grad, use_thread_group)
        self.gen_add_end_control_flow()
        if staged:
            self.gen_kernel_save_result("d2eePos", hess, hess, use_thread_group)
    self.gen_add_end_control_flow()
    self.gen_add_end_function()


def gen_end_effector_pose_kernel(self, use_thread_group=False):
    _ee_kernel(self, 0, use_thread_group)


def gen_end_effector_pose_gradient_kernel(self, use_thread_group=False):
    _ee_kernel(self, 1, use_thread_group)


def gen_end_effector_pose_gradient_hessian_kernel(self, use_thread_group=False):
    _ee_kernel(self, 2, use_thread_group)


def _ee_host(self, kind, mode=0):
    single_call_timing = mode == 1
    compute_only = mode == 2
    name, C = _EE_KINDS[kind]
    outs = {0: [("eePos", "6*NUM_EES")], 1: [("deePos", "6*NUM_EES*NUM_JOINTS")],
            2: [("d2eePos", "6*NUM_EES*NUM_JOINTS*NUM_JOINTS"), ("deePos", "6*NUM_EES*NUM_JOINTS")]}[kind]
    func_params = ["hd_data is the packaged input and output pointers (its kinematics buffers are allocated by the first call and grown by longer ones)",
                   "d_robotModel is the pointer to the initialized model specific helpers on the GPU",
                   "num_timesteps is the length of the trajectory points we need to compute over (or overloaded as test_iters for timing)",
                   "streams are pointers to HIP streams for async memory transfers (if needed)"]
    fname = name + ("_single_timing" if single_call_timing else "") + ("_compute_only" if compute_only else "")
    self.gen_add_func_doc("Compute " + name.replace("_", " "),
                          ["USE_COMPRESSED_MEM: q is read from d_q / h_q (stride n), otherwise from d_q_qd_u / h_q_qd_u (stride 3n)",
                           "_single_timing: one solve, num_timesteps launches of one lane group, time per launch printed"] if mode == 0 else [], func_params, None)
    self.gen_add_code_line("template <typename T, bool USE_COMPRESSED_MEM = false>")
    self.gen_add_code_line("__host__")
    self.gen_add_code_line("void " + fname + "(gridData<T> *hd_data, const robotModel<T> *d_robotModel, const int num_timesteps,")
    self.gen_add_code_line("                      const dim3 block_dimms, const dim3 thread_dimms" + ("" if compute_only else ", hipStream_t *streams") + ") {", True)
    cnt = "1" if single_call_timing else "num_timesteps"
    for nm, sz in outs:
        self.gen_add_code_line("grid_ee_reserve<T>(&hd_data->d_%s, &hd_data->h_%s, %s, %s);" % (nm, nm, sz, cnt))
    self.gen_add_code_lines(["const int stride_q = USE_COMPRESSED_MEM ? NUM_JOINTS : 3*NUM_JOINTS;",
                             "T *d_q = USE_COMPRESSED_MEM ? hd_data->d_q : hd_data->d_q_qd_u;"])
    if not compute_only:
        self.gen_add_code_lines(["// start code with memory transfer",
                                 "gpuErrchk(hipMemcpyAsync(d_q, USE_COMPRESSED_MEM ? hd_data->h_q : hd_data->h_q_qd_u, stride_q*" + cnt + "*sizeof(T), hipMemcpyHostToDevice, streams[0]));",
                                 "gpuErrchk(hipDeviceSynchronize());"])
    args = ",".join("hd_data->d_" + nm for nm, _ in outs)
    self.gen_add_code_line("// then call the kernel")
    if single_call_timing:
        self.gen_add_code_lines(["struct timespec start, end; clock_gettime(CLOCK_MONOTONIC,&start);",
                                 "const dim3 one_group(GRID_MIN_THREADS);",
                                 "for (int rep = 0; rep < num_timesteps; rep++) {",
                                 "    hipLaunchKernelGGL((%s_kernel<T>),dim3(1),one_group,grid_lds_bytes<T>(one_group, %s_LDS_PER_SOLVE, %s_OUT_PER_SOLVE),0,%s,d_q,stride_q,d_robotModel,1);" % (name, C, C, args),
                                 "}",
                                 "gpuErrchk(hipGetLastError()); gpuErrchk(hipDeviceSynchronize());",
                                 "clock_gettime(CLOCK_MONOTONIC,&end);"])
    else:
        self.gen_add_code_lines(["hipLaunchKernelGGL((%s_kernel<T>),block_dimms,thread_dimms,grid_lds_bytes<T>(thread_dimms, %s_LDS_PER_SOLVE, %s_OUT_PER_SOLVE),0,%s,d_q,stride_q,d_robotModel,num_timesteps);" % (name, C, C, args),
                                 "gpuErrchk(hipGetLastError()); gpuErrchk(hipDeviceSynchronize());"])
    if not compute_only:
        self.gen_add_code_line("// finally transfer the result back")
        for nm, sz in outs:
            self.gen_add_code_line("gpuErrchk(hipMemcpy(hd_data->h_%s,hd_data->d_%s,static_cast<size_t>(%s)*%s*sizeof(T),hipMemcpyDeviceToHost));" % (nm, nm, sz, cnt))
        self.gen_add_code_line("gpuErrchk(hipDeviceSynchronize());")
    if single_call_timing:
        self.gen_add_code_line("printf(\"Single Call %s %%fus\\n\",time_delta_us_timespec(start,end)/static_cast<double>(num_timesteps));" % name.replace("_", " ").upper())
    self.gen_add_end_function()


def gen_end_effector_pose_host(self, mode=0):
    _ee_host(self, 0, mode)


def gen_end_effector_pose_gradient_host(self, mode=0):
    _ee_host(self, 1, mode)


def gen_end_effector_pose_gradient_hessian_host(self, mode=0):
    _ee_host(self, 2, mode)


def gen_eepose_buffers(self):
    self.gen_add_func_doc("Allocates (or grows) one kinematics output buffer of gridData: device + pinned host memory for num_timesteps solves",
                          ["init_gridData leaves d_/h_eePos, deePos, d2eePos null (a 30-DoF Hessian for 16 384 solves would be 1.8 GB of each): the kinematics host",
                           "wrappers allocate them on first use, sized for that call, and grow them when a later call is longer; close_grid frees them.",
                           "The capacity (solves) is kept in the 16 bytes in front of the pinned host buffer."], [], None)
    self.gen_add_code_lines(["template <typename T>",
                             "__host__ inline void grid_ee_reserve(T **d_buf, T **h_buf, const int per_solve, const int num_timesteps) {",
                             "    const int want = num_timesteps > 1 ? num_timesteps : 1;",
                             "    if (*h_buf != nullptr && reinterpret_cast<const int *>(*h_buf)[-4] >= want) {return;}",
                             "    if (*d_buf != nullptr) {gpuErrchk(hipFree(*d_buf)); *d_buf = nullptr;}",
                             "    if (*h_buf != nullptr) {gpuErrchk(hipHostFree(reinterpret_cast<char *>(*h_buf) - 16)); *h_buf = nullptr;}",
                             "    const size_t bytes = static_cast<size_t>(per_solve)*want*sizeof(T);",
                             "    gpuErrchk(hipMalloc((void**)d_buf, bytes));",
                             "    char *hb = nullptr; gpuErrchk(hipHostMalloc((void**)&hb, 16 + bytes, hipHostMallocDefault));",
                             "    reinterpret_cast<int *>(hb)[0] = want;",
                             "    *h_buf = reinterpret_cast<T *>(hb + 16);",
                             "}",
                             "template <typename T>",
                             "__host__ inline void grid_ee_release(T **d_buf, T **h_buf) {",
                             "    if (*d_buf != nullptr) {gpuErrchk(hipFree(*d_buf)); *d_buf = nullptr;}",
                             "    if (*h_buf != nullptr) {gpuErrchk(hipHostFree(reinterpret_cast<char *>(*h_buf) - 16)); *h_buf = nullptr;}",
                             "}", ""])


def gen_eepose_and_derivatives(self, use_thread_group=False):
    self.gen_eepose_constants()
    self.gen_eepose_buffers()
    self.gen_end_effector_pose_inner(use_thread_group)
    self.gen_end_effector_pose_device(use_thread_group)
    self.gen_end_effector_pose_kernel(use_thread_group)
    self.gen_end_effector_pose_gradient_inner(use_thread_group)
    self.gen_end_effector_pose_gradient_device(use_thread_group)
    self.gen_end_effector_pose_gradient_kernel(use_thread_group)
    self.gen_end_effector_pose_gradient_hessian_inner(use_thread_group)
    self.gen_end_effector_pose_gradient_hessian_device(use_thread_group)
    self.gen_end_effector_pose_gradient_hessian_kernel(use_thread_group)
    for mode in (0, 1, 2):
        self.gen_end_effector_pose_host(mode)
        self.gen_end_effector_pose_gradient_host(mode)
        self.gen_end_effector_pose_gradient_hessian_host(mode)
