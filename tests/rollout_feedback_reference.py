"""The reference every closed-loop rollout test compares against: the fp64 oracle (oracle.rbd_oracle) stepped in NumPy fp64 with the feedback law, the clamp and the
three update lines written out here - none of the code under test.  Per solve and step:
    dx = x_t - x_ref[t];  v = u_ff[t] + sum_c K[t][c*n + j] dx[c];  u_t = v, or v < u_min ? u_min : (v > u_max ? u_max : v);
    qdd = FD(q_t, qd_t, u_t);  qd_{t+1} = qd_t + dt qdd;  q_{t+1} = q_t + dt qd_{t+1}
Inputs: "gentle" (x0, x_ref ~ U(-1, 1), u_ff ~ U(-5, 5), K = -[1 I | 0.02 I] + U(-0.02, 0.02), limits +-4: about a fifth of the applied controls saturate) for every
fixture; "strong" (K = -[20 I | 2 I] + U(-1, 1), limits +-30) for hyq, mixed5 and chain8 only: on the other fixtures these gains diverge in the fp64 oracle itself
(light distal links: dt Kd M^-1 > 2).  Every entry of K is non-zero, so a transposed or mis-strided record changes u by far more than the bar."""
import numpy as np

from gridcodegenerator_amd import RobotModel
from oracle.rbd_oracle import Oracle

STRONG_FIXTURES = ["hyq", "mixed5", "chain8"]
GENTLE = dict(kp=1.0, kd=0.02, noise=0.02, limit=4.0)
STRONG = dict(kp=20.0, kd=2.0, noise=1.0, limit=30.0)


def _expand(a, T, N, rec):
    """(T, N, rec) view of a dense, solve-shared or fully shared record array"""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        return np.broadcast_to(a, (T, N, rec))
    if a.ndim == 2:
        return np.broadcast_to(a[:T, None, :], (T, N, rec))
    return a[:T]


def oracle_rollout_feedback(robot, x0, u_ff, K, x_ref, dt, u_min=None, u_max=None, gravity=9.81):
    """x0 (N, >= 2n), u_ff (T, N, n) or (T, n), K (T, N, 2n^2) / (T, 2n^2) / (2n^2,) records [c*n + j], x_ref (>= T, N, 2n) / (>= T, 2n) / (2n,),
    u_min / u_max scalars or (n,) -> (traj (T+1, N, 2n), u_applied (T, N, n)) in float64"""
    if isinstance(robot, str):
        robot = RobotModel.from_fixture(robot)
    o = Oracle(robot)
    n = o.n
    x0 = np.asarray(x0, np.float64)
    u_ff = np.asarray(u_ff, np.float64)
    N, T = x0.shape[0], u_ff.shape[0]
    if u_ff.ndim == 2:
        u_ff = np.broadcast_to(u_ff[:, None, :], (T, N, n))
    K = _expand(K, T, N, 2 * n * n)
    x_ref = _expand(x_ref, T, N, 2 * n)
    lo = None if u_min is None else np.broadcast_to(np.asarray(u_min, np.float64), (n,))
    hi = None if u_max is None else np.broadcast_to(np.asarray(u_max, np.float64), (n,))
    traj, applied = np.zeros((T + 1, N, 2 * n)), np.zeros((T, N, n))
    traj[0] = x0[:, :2 * n]
    for k in range(N):
        q, qd = x0[k, :n].copy(), x0[k, n:2 * n].copy()
        for t in range(T):
            dx = np.concatenate([q, qd]) - x_ref[t, k]
            v = u_ff[t, k] + K[t, k].reshape(2 * n, n).T @ dx
            if lo is not None:
                v = np.where(v < lo, lo, np.where(v > hi, hi, v))
            applied[t, k] = v
            qdd = o.fd_grad(q, qd, v, gravity, full=True)[1]
            qd = qd + dt * qdd
            q = q + dt * qd
            traj[t + 1, k, :n], traj[t + 1, k, n:] = q, qd
    return traj, applied


def per_solve_err_u(got, ref):
    """max|got - ref| / max(1, max|ref|) over a solve's (t, j); got / ref: (T, N, n) -> (N,).  NaN or inf on either side gives inf."""
    from rollout_reference import per_solve_err

    return per_solve_err(got, ref)


def feedback_inputs(n, N, T, seed, dtype=np.float32, kind=GENTLE):
    """(x0 (N, 2n), u_ff (T, N, n), K (T, N, 2n^2) records, x_ref (T, N, 2n), limit)"""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1, 1, (N, 2 * n))
    u_ff = rng.uniform(-5, 5, (T, N, n))
    x_ref = rng.uniform(-1, 1, (T, N, 2 * n))
    Kmat = -np.hstack([kind["kp"] * np.eye(n), kind["kd"] * np.eye(n)]) + rng.uniform(-kind["noise"], kind["noise"], (T, N, n, 2 * n))  # row-major (n, 2n)
    K = np.ascontiguousarray(np.swapaxes(Kmat, -1, -2)).reshape(T, N, 2 * n * n)  # records [c*n + j]
    return x0.astype(dtype), u_ff.astype(dtype), K.astype(dtype), x_ref.astype(dtype), kind["limit"]
