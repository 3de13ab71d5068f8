"""NumPy reference implementations bound to the generator object, like the reference's `_test.py` (README "Additional
Features": test_rnea :109, test_minv :213, test_rnea_grad :490, test_fd_grad :496).  They are DEBUG HELPERS for users who want to
compare device output by hand; nothing on the GPU path (kernels, C ABI, bench, tests) calls them - the tests use the separate
checker in oracle/ and the reference-generated goldens.  Same signatures and conventions as the reference: GRAVITY = -9.81
(negated internally), outputs (c, v, a, f) with 6 x n arrays, dc_du = hstack(dc_dq, dc_dqd), df_du = -Minv dc_du.

Written as plain recursions over the kinematic tree (children fold into parents) on the generator's numeric model.
"""
import numpy as np


def _mxS(s, vec, alpha=1.0):
    """alpha * crm(vec) * e_s"""
    out = np.zeros(6)
    crm = _crm(vec)
    out[:] = crm[:, s] * alpha
    return out


def _crm(v):
    w, l = v[:3], v[3:]
    sk = lambda x: np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
    out = np.zeros((6, 6))
    out[:3, :3] = sk(w)
    out[3:, :3] = sk(l)
    out[3:, 3:] = sk(w)
    return out


def _crf(v):
    return -_crm(v).T


def _Xs(self, q):
    m = self.model
    return [m.X(j, float(q[j])) for j in range(m.n)]


def test_rnea(self, q, qd, qdd=None, GRAVITY=-9.81):
    m = self.model
    n = m.n
    X = _Xs(self, q)
    v, a, f = np.zeros((6, n)), np.zeros((6, n)), np.zeros((6, n))
    a_base = np.zeros(6)
    a_base[5] = -GRAVITY
    for j in range(n):  # ids are parent-first
        p, s = m.parent[j], m.S_index[j]
        vp = v[:, p] if p != -1 else np.zeros(6)
        ap = a[:, p] if p != -1 else a_base
        v[:, j] = X[j] @ vp
        v[s, j] += qd[j]
        a[:, j] = X[j] @ ap + _mxS(s, v[:, j], qd[j])
        if qdd is not None:
            a[s, j] += qdd[j]
        f[:, j] = m.I[j] @ a[:, j] + _crf(v[:, j]) @ (m.I[j] @ v[:, j])
    c = np.zeros(n)
    for j in range(n - 1, -1, -1):
        c[j] = f[m.S_index[j], j] + m.damping[j] * qd[j]
        if m.parent[j] != -1:
            f[:, m.parent[j]] += X[j].T @ f[:, j]
    return (c, v, a, f)


def test_minv(self, q, output_dense=True):
    m = self.model
    n = m.n
    X = _Xs(self, q)
    IA = [m.I[j].copy() for j in range(n)]
    F = [np.zeros((6, n)) for _ in range(n)]
    U, Dinv, Minv = np.zeros((n, 6)), np.zeros(n), np.zeros((n, n))
    for j in range(n - 1, -1, -1):
        s, p = m.S_index[j], m.parent[j]
        U[j] = IA[j][:, s]
        Dinv[j] = 1.0 / U[j, s]
        sub = m.subtree[j]
        Minv[j, j] = Dinv[j]
        Minv[j, sub] -= Dinv[j] * F[j][s, sub]
        if p != -1:
            F[j][:, sub] += np.outer(U[j], Minv[j, sub])
            F[p][:, sub] += X[j].T @ F[j][:, sub]
            IA[p] += X[j].T @ (IA[j] - np.outer(U[j], U[j]) * Dinv[j]) @ X[j]
    for j in range(n):
        s, p = m.S_index[j], m.parent[j]
        if p != -1:
            Minv[j, j:] -= Dinv[j] * (U[j] @ X[j]) @ F[p][:, j:]
        F[j][:, j:] = 0.0
        F[j][s, j:] = Minv[j, j:]
        if p != -1:
            F[j][:, j:] += X[j] @ F[p][:, j:]
    if output_dense:
        Minv = np.triu(Minv) + np.triu(Minv, 1).T
    return Minv


def test_rnea_grad(self, q, qd, qdd=None, GRAVITY=-9.81):
    """dc_du (n x 2n) by the same forward-accumulation identity the generated kernels use:
    dc[a][col] = sum_k J_{k,a} . df_k[col] minus the S^T-projection of the propagated mxS(S, f_subtree) corrections."""
    m = self.model
    n = m.n
    X = _Xs(self, q)
    c, v, a, f = test_rnea(self, q, qd, qdd, GRAVITY)  # f is the accumulated subtree force
    a_base = np.zeros(6)
    a_base[5] = -GRAVITY
    dv, da = np.zeros((n, 6, 2 * n)), np.zeros((n, 6, 2 * n))
    dc = np.zeros((n, 2 * n))
    for k in range(n):
        s, p = m.S_index[k], m.parent[k]
        ap = a[:, p] if p != -1 else a_base
        if p != -1:
            dv[k] = X[k] @ dv[p]
            da[k] = X[k] @ da[p]
        dv[k][:, k] += _mxS(s, v[:, k])
        dv[k][s, n + k] += 1.0
        da[k][:, k] += _mxS(s, X[k] @ ap)
        da[k][:, n + k] += _mxS(s, v[:, k])
        for col in range(2 * n):
            da[k][:, col] += _mxS(s, dv[k][:, col], qd[k])
        Iv = m.I[k] @ v[:, k]
        df = m.I[k] @ da[k] + _crf(v[:, k]) @ (m.I[k] @ dv[k])
        for col in range(2 * n):
            df[:, col] += _crf(dv[k][:, col]) @ Iv
        for anc in m.ancestors[k] + [k]:
            dc[anc] += dv[k][:, n + anc] @ df  # J_{k,anc} = d v_k / d qd_anc
    for i in range(n):  # corrections of column q_i travel from joint i to the root
        w = _mxS(m.S_index[i], f[:, i])
        j = i
        while m.parent[j] != -1:
            w = X[j].T @ w
            j = m.parent[j]
            dc[j, i] -= w[m.S_index[j]]
    for i in range(n):
        dc[i, n + i] += m.damping[i]
    return dc


def test_fd_grad(self, q, qd, u, GRAVITY=-9.81):
    c = test_rnea(self, q, qd, None, GRAVITY)[0]
    Minv = test_minv(self, q, True)
    qdd = Minv @ (np.asarray(u) - c)
    return -Minv @ test_rnea_grad(self, q, qd, qdd, GRAVITY)


# ---------------------------------------------------------------------------------------------------- end-effector kinematics
# From the joint descriptions alone (xyz, rpy, axis, type of every joint; reference algorithms/_eepose_gradient_hessian.py): T_e(q) = T_root ... T_leaf with
# T_j(q) = [R_tree_j Rot(axis_j, q) | xyz_j] (revolute) or [R_tree_j | xyz_j + R_tree_j axis_j q] (prismatic), pose [x, y, z, roll, pitch, yaw],
# roll = atan2(R21, R22), pitch = -atan2(R20, sqrt(R21^2 + R22^2)), yaw = atan2(R10, R00).  The derivatives are analytic (products of the joint transforms
# with their derivatives), so the tests can pin them against finite differences.  Layouts: (E, 6), (E, 6, n) and (E, 6, n, n).

def _rpy_matrix(rpy):
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def _ee_joints(self):
    """(parent, xyz, R_tree, axis index, revolute) of every joint, from the robot's own joint descriptions"""
    out = []
    for jt in self.robot.get_joints_ordered_by_id():
        out.append((int(jt.parent), np.asarray(jt.xyz, float), _rpy_matrix(jt.rpy), int(jt.axis), jt.jtype == "revolute"))
    return out


def _ee_local(J, q, order):
    """4x4 homogeneous transform of one joint and its first and second derivative in q (order 0, 1, 2)"""
    _, xyz, Rt, a, rev = J
    T = np.zeros((4, 4))
    if rev:
        K = np.zeros((3, 3))
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        K[a2, a1], K[a1, a2] = 1.0, -1.0  # skew(e_a)
        c, s = np.cos(q), np.sin(q)
        Rot = np.eye(3) + s * K + (1 - c) * K @ K
        dRot = [Rot, c * K + s * K @ K, -s * K + c * K @ K][order]
        T[:3, :3] = Rt @ dRot
        if order == 0:
            T[:3, 3] = xyz
            T[3, 3] = 1.0
    else:
        if order == 0:
            T[:3, :3] = Rt
            T[:3, 3] = xyz + Rt[:, a] * q
            T[3, 3] = 1.0
        elif order == 1:
            T[:3, 3] = Rt[:, a]
    return T


def _ee_leaves(self):
    m = self.model
    return [j for j in range(m.n) if not m.children[j]]


def _ee_path(joints, leaf):
    path = []
    j = leaf
    while j != -1:
        path.append(j)
        j = joints[j][0]
    return path[::-1]


def _ee_chain(joints, q, path, d):
    """product over the root path with joint path[k] differentiated d[k] times"""
    T = np.eye(4)
    for k, j in enumerate(path):
        T = T @ _ee_local(joints[j], float(q[j]), d.get(j, 0))
    return T


def _atan2_derivs(y, x, dy, dx, d2y=None, d2x=None):
    """first (n) and second (n x n) derivatives of atan2(y, x) from those of y and x"""
    D = x * x + y * y
    g = (x * dy - y * dx) / D
    if d2y is None:
        return g
    dD = 2 * (x * dx + y * dy)
    H = (np.outer(dy, dx) + x * d2y - np.outer(dx, dy) - y * d2x) / D - np.outer(x * dy - y * dx, dD) / D ** 2
    return g, H


def _ee_all(self, q, order):
    joints = _ee_joints(self)
    n = len(joints)
    q = np.asarray(q, float)
    leaves = _ee_leaves(self)
    E = len(leaves)
    pose, grad, hess = np.zeros((E, 6)), np.zeros((E, 6, n)), np.zeros((E, 6, n, n))
    for e, leaf in enumerate(leaves):
        path = _ee_path(joints, leaf)
        T = _ee_chain(joints, q, path, {})
        dT = np.zeros((n, 4, 4))
        d2T = np.zeros((n, n, 4, 4))
        if order >= 1:
            for i in path:
                dT[i] = _ee_chain(joints, q, path, {i: 1})
        if order >= 2:
            for i in path:
                for j in path:
                    d2T[i, j] = _ee_chain(joints, q, path, {i: 2} if i == j else {i: 1, j: 1})
        R, p = T[:3, :3], T[:3, 3]
        s = np.hypot(R[2, 1], R[2, 2])
        pose[e] = [p[0], p[1], p[2], np.arctan2(R[2, 1], R[2, 2]), -np.arctan2(R[2, 0], s), np.arctan2(R[1, 0], R[0, 0])]
        if order == 0:
            continue
        el = lambda r, c: (dT[:, r, c], d2T[:, :, r, c])
        (d21, h21), (d22, h22), (d20, h20), (d10, h10), (d00, h00) = el(2, 1), el(2, 2), el(2, 0), el(1, 0), el(0, 0)
        ds = (R[2, 1] * d21 + R[2, 2] * d22) / s
        h_s = (np.outer(d21, d21) + R[2, 1] * h21 + np.outer(d22, d22) + R[2, 2] * h22) / s - np.outer(ds, ds) / s
        grad[e, :3] = dT[:, :3, 3].T
        hess[e, :3] = np.moveaxis(d2T[:, :, :3, 3], 2, 0)
        for c, (y, x, dy, dx, hy, hx, sign) in enumerate([(R[2, 1], R[2, 2], d21, d22, h21, h22, 1.0), (R[2, 0], s, d20, ds, h20, h_s, -1.0),
                                                          (R[1, 0], R[0, 0], d10, d00, h10, h00, 1.0)]):
            g, H = _atan2_derivs(y, x, dy, dx, hy, hx)
            grad[e, 3 + c] = sign * g
            hess[e, 3 + c] = sign * 0.5 * (H + H.T)
    return pose, grad, hess


def test_end_effector_pose(self, q):
    """(E, 6): [x, y, z, roll, pitch, yaw] of every leaf joint (ascending id)"""
    return _ee_all(self, q, 0)[0]


def test_end_effector_pose_gradient(self, q):
    """(E, 6, n): d pose / d q_j (0 for joints off the leaf's root path)"""
    return _ee_all(self, q, 1)[1]


def test_end_effector_pose_hessian(self, q):
    """(E, 6, n, n): d2 pose / d q_i d q_j (symmetric; 0 unless both joints are on the leaf's root path)"""
    return _ee_all(self, q, 2)[2]


def test_crba(self, q):
    """(n, n): the joint-space inertia matrix M(q) by the composite rigid body algorithm (dense, symmetric; 0 where neither joint is an
    ancestor of the other).  Composites fold into parents leaves first; F = I^C_j S_j walks up the root path of j."""
    m = self.model
    n = m.n
    X = _Xs(self, q)
    IC = [m.I[j].copy() for j in range(n)]
    M = np.zeros((n, n))
    for j in range(n - 1, -1, -1):  # (ids are parent-first: every child is folded in before its parent is reached)
        p = m.parent[j]
        if p != -1:
            IC[p] += X[j].T @ IC[j] @ X[j]
    for j in range(n):
        F = IC[j][:, m.S_index[j]].copy()
        M[j, j] = F[m.S_index[j]]
        i = j
        while m.parent[i] != -1:
            F = X[i].T @ F
            i = m.parent[i]
            M[i, j] = M[j, i] = F[m.S_index[i]]
    return M


def test_rollout(self, q, qd, U, dt, GRAVITY=-9.81):
    """(T+1, 2n): the states [q_t | qd_t] of T = len(U) steps of semi-implicit (symplectic) Euler from (q, qd) under the controls U (T, n), row 0 being the
    start: qdd = Minv(q_t) (u_t - c(q_t, qd_t)), qd_{t+1} = qd_t + dt qdd, q_{t+1} = q_t + dt qd_{t+1} (the NEW velocity).  No joint limits, no angle
    wrapping, no contact: what rollout_kernel computes, in fp64."""
    q, qd = np.array(q, float), np.array(qd, float)
    U = np.asarray(U, float).reshape(-1, self.model.n)
    traj = np.zeros((len(U) + 1, 2 * self.model.n))
    traj[0] = np.concatenate([q, qd])
    for t, u in enumerate(U):
        qdd = test_minv(self, q, True) @ (u - test_rnea(self, q, qd, None, GRAVITY)[0])
        qd = qd + dt * qdd
        q = q + dt * qd
        traj[t + 1] = np.concatenate([q, qd])
    return traj


def test_rollout_linearized(self, q, qd, U, dt, GRAVITY=-9.81):
    """(states (T+1, 2n), fx (T, 2n^2), fu (T, n^2)): test_rollout's states and, at every (q_t, qd_t, u_t) along them, the records rollout_linearized_kernel
    writes: fx = test_fd_grad (n x 2n, stored fx[col*n + row]) and fu = d qdd/du = test_minv (dense, symmetric, fu[col*n + row]), in fp64."""
    n = self.model.n
    U = np.asarray(U, float).reshape(-1, n)
    traj = test_rollout(self, q, qd, U, dt, GRAVITY)
    fx, fu = np.zeros((len(U), 2 * n * n)), np.zeros((len(U), n * n))
    for t, u in enumerate(U):
        fx[t] = test_fd_grad(self, traj[t, :n], traj[t, n:], u, GRAVITY).T.reshape(-1)
        Minv = test_minv(self, traj[t, :n], True)
        fu[t] = (0.5 * (Minv + Minv.T)).T.reshape(-1)
    return traj, fx, fu


def test_rollout_adjoint(self, traj, U, dt, gx=None, gxT=None, GRAVITY=-9.81):
    """(grad_x0 (2n), grad_u (T, n)): the gradient of L = sum_t <gx[t], x_t> (+ <gxT, x_T>) with respect to x0 and every u_t along the stored states traj (T+1, 2n)
    of test_rollout under U (T, n): lam_T = gx[T] (+ gxT); for t = T-1 .. 0, with [Fq | Fv] = test_fd_grad and M^-1 = test_minv at (traj[t], U[t]),
        w = lv + dt lq;  grad_u_t = dt M^-1 w;  lq <- gx[t, :n] + lq + dt Fq^T w;  lv <- gx[t, n:] + w + dt Fv^T w
    what rollout_adjoint_kernel computes, in fp64."""
    n = self.model.n
    U = np.asarray(U, float).reshape(-1, n)
    traj = np.asarray(traj, float).reshape(len(U) + 1, 2 * n)
    g = np.zeros((len(U) + 1, 2 * n)) if gx is None else np.array(gx, float).reshape(len(U) + 1, 2 * n)
    if gxT is not None:
        g[-1] += np.asarray(gxT, float).reshape(2 * n)
    lq, lv = g[-1, :n].copy(), g[-1, n:].copy()
    grad_u = np.zeros((len(U), n))
    for t in range(len(U) - 1, -1, -1):
        F = test_fd_grad(self, traj[t, :n], traj[t, n:], U[t], GRAVITY)  # (n, 2n)
        Minv = test_minv(self, traj[t, :n], True)
        w = lv + dt * lq
        grad_u[t] = dt * (0.5 * (Minv + Minv.T) @ w)
        lq, lv = g[t, :n] + lq + dt * (F[:, :n].T @ w), g[t, n:] + w + dt * (F[:, n:].T @ w)
    return np.concatenate([lq, lv]), grad_u


def test_rollout_feedback(self, q, qd, U_ff, K, X_ref, dt, u_min=None, u_max=None, GRAVITY=-9.81):
    """(states (T+1, 2n), applied controls (T, n)): test_rollout's integrator under the closed-loop law of rollout_feedback_kernel, in fp64.  U_ff (T, n), K (T, 2n^2)
    records K[c*n + j] (or one record (2n^2,) for all steps), X_ref (>= T, 2n) (or one set point (2n,)), u_min / u_max (n,) both or neither:
        u_t = clamp(U_ff[t] + K_t (x_t - X_ref[t]));  qdd = Minv(q_t) (u_t - c(q_t, qd_t));  qd_{t+1} = qd_t + dt qdd;  q_{t+1} = q_t + dt qd_{t+1}
    with one accumulator per joint that starts from U_ff and takes the columns of K in ascending order, and the clamp v < u_min ? u_min : (v > u_max ? u_max : v)."""
    n = self.model.n
    q, qd = np.array(q, float), np.array(qd, float)
    U_ff = np.asarray(U_ff, float).reshape(-1, n)
    T = len(U_ff)
    K = np.broadcast_to(np.asarray(K, float).reshape(-1, 2 * n * n), (T, 2 * n * n)) if np.size(K) == 2 * n * n else np.asarray(K, float).reshape(T, 2 * n * n)
    X_ref = np.broadcast_to(np.asarray(X_ref, float).reshape(2 * n), (T, 2 * n)) if np.size(X_ref) == 2 * n else np.asarray(X_ref, float).reshape(-1, 2 * n)
    if (u_min is None) != (u_max is None):
        raise ValueError("u_min and u_max come together")
    traj, applied = np.zeros((T + 1, 2 * n)), np.zeros((T, n))
    traj[0] = np.concatenate([q, qd])
    for t in range(T):
        dx = traj[t] - X_ref[t]
        v = U_ff[t].copy()
        for c in range(2 * n):
            v = v + K[t, c * n:(c + 1) * n] * dx[c]
        if u_min is not None:
            lo, hi = np.asarray(u_min, float), np.asarray(u_max, float)
            v = np.where(v < lo, lo, np.where(v > hi, hi, v))
        applied[t] = v
        qdd = test_minv(self, q, True) @ (v - test_rnea(self, q, qd, None, GRAVITY)[0])
        qd = qd + dt * qdd
        q = q + dt * qd
        traj[t + 1] = np.concatenate([q, qd])
    return traj, applied
