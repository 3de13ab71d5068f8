"""The reference of every linearised-rollout test: the fp64 oracle (oracle.rbd_oracle) and NumPy, none of the code under test.

States: rollout_reference.oracle_rollout.  Jacobians: Oracle.fd_grad(q, qd, u, full=True) -> (df_du, qdd, Minv dense, ...), evaluated AT THE STATE THE CODE
UNDER TEST RETURNED (traj[t, k] cast to fp64) with u[t, k] - so a Jacobian check measures the Jacobian, not trajectory drift times second derivatives.
Only the inputs of the reference come from the kernel; every reference value comes from the oracle.

Bars (tests/test_gpu_parity.py): per record max|got - ref| <= 1e-4 * max|ref| in fp32, 1e-9 in fp64; fx and fu each on their own;
NaN / inf on either side fails."""
import numpy as np

from gridcodegenerator_amd import RobotModel
from oracle.rbd_oracle import Oracle

JTOL32, JTOL64 = 1e-4, 1e-9


def oracle_jacobians(robot, traj, u, gravity=9.81, dtype=np.float64):
    """traj (T+1, N, 2n) (any float type), u (T, N, n) or (T, n) -> fx (T, N, 2n^2), fu (T, N, n^2) in fp64, record layouts of the library ([col*n + row])"""
    if isinstance(robot, str):
        robot = RobotModel.from_fixture(robot)
    o = Oracle(robot, dtype) if dtype is not np.float64 else Oracle(robot)
    n = o.n
    traj = np.asarray(traj, np.float64)
    u = np.asarray(u, np.float64)
    T, N = u.shape[0], traj.shape[1]
    if u.ndim == 2:
        u = np.broadcast_to(u[:, None, :], (T, N, n))
    fx, fu = np.zeros((T, N, 2 * n * n)), np.zeros((T, N, n * n))
    for t in range(T):
        for k in range(N):
            if not np.isfinite(traj[t, k]).all():
                fx[t, k], fu[t, k] = np.nan, np.nan
                continue
            with np.errstate(all="ignore"):
                res = o.fd_grad(traj[t, k, :n].astype(dtype), traj[t, k, n:].astype(dtype), u[t, k].astype(dtype), gravity, full=True)
            fx[t, k] = np.asarray(res[0], np.float64).reshape(n, 2 * n).T.reshape(-1)
            fu[t, k] = np.asarray(res[2], np.float64).reshape(n, n).T.reshape(-1)
    return fx, fu


def per_record_err(got, ref):
    """max|got - ref| / max|ref| of every record; got / ref (..., R) -> (...).  NaN or inf on either side gives inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        e = np.abs(got - ref).max(axis=-1) / np.abs(ref).max(axis=-1)
    bad = ~(np.isfinite(got).all(axis=-1) & np.isfinite(ref).all(axis=-1))
    return np.where(bad | ~np.isfinite(e), np.inf, e)


def block_jacobians(fx, fu, dt):
    """A (2n, 2n), B (2n, n) of ONE record pair from the block formula, written out with explicit indices (the statement discrete_jacobians is tested against)"""
    n = int(round(fu.size ** 0.5))
    Fq = np.array([[fx[c * n + r] for c in range(n)] for r in range(n)])
    Fv = np.array([[fx[(n + c) * n + r] for c in range(n)] for r in range(n)])
    Mi = np.array([[fu[c * n + r] for c in range(n)] for r in range(n)])
    I = np.eye(n)
    A = np.block([[I + dt * dt * Fq, dt * (I + dt * Fv)], [dt * Fq, I + dt * Fv]])
    B = np.vstack([dt * dt * Mi, dt * Mi])
    return A, B
