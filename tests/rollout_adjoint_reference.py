"""The reference of every rollout-adjoint test: the fp64 oracle (oracle.rbd_oracle) and NumPy, none of the code under test.

For every step the discrete Jacobians A_t, B_t are built with rollout_linearized_reference.block_jacobians from oracle_jacobians evaluated AT THE traj AND u
HANDED TO THE CODE UNDER TEST (traj is an input of the adjoint: reference and kernel see the same states).  Then the un-collapsed recurrence runs in fp64:
    lam_T = g_T;   t = T-1 .. 0:  grad_u_t = B_t^T lam_{t+1},  lam_t = g_t + A_t^T lam_{t+1};   grad_x0 = lam_0

Error per solve: max|got - ref| / max|ref| over the solve's grad_x0 record, and over all (t, j) of its grad_u, each on its own; NaN or inf on either side fails.
Bars: the project's 1e-4 (fp32) and 1e-9 (fp64).  Inputs: rollout_reference.inputs, g ~ U(-1, 1) at every step (no reference record is near zero), dt = 1 ms."""
import numpy as np

from rollout_linearized_reference import block_jacobians, oracle_jacobians

ATOL32, ATOL64 = 1e-4, 1e-9
DT = 1e-3


def cotangent(n, N, T, seed, dtype=np.float32):
    """g ~ U(-1, 1), (T+1, N, 2n)"""
    return np.random.default_rng(1000 + seed).uniform(-1, 1, (T + 1, N, 2 * n)).astype(dtype)


def oracle_adjoint(robot, traj, u, dt, gx=None, gxT=None, gravity=9.81, dtype=np.float64):
    """traj (T+1, N, 2n), u (T, N, n) or (T, n), gx (T+1, N, 2n) and / or gxT (N, 2n) -> grad_x0 (N, 2n), grad_u (T, N, n) in fp64 (per solve, also for shared u)"""
    traj = np.asarray(traj, np.float64)
    T, N = traj.shape[0] - 1, traj.shape[1]
    n = traj.shape[2] // 2
    g = np.zeros_like(traj) if gx is None else np.array(gx, np.float64)
    if gxT is not None:
        g[T] = g[T] + np.asarray(gxT, np.float64)
    fx, fu = oracle_jacobians(robot, traj, u, gravity, dtype) if T > 0 else (None, None)
    grad_x0, grad_u = np.zeros((N, 2 * n)), np.zeros((T, N, n))
    for k in range(N):
        lam = g[T, k].copy()
        for t in range(T - 1, -1, -1):
            A, B = block_jacobians(fx[t, k], fu[t, k], dt)
            with np.errstate(all="ignore"):
                grad_u[t, k] = B.T @ lam
                lam = g[t, k] + A.T @ lam
        grad_x0[k] = lam
    return grad_x0, grad_u


def per_solve_err(got, ref):
    """got / ref: grad_x0 (N, 2n) or grad_u (T, N, n) -> (N,): max|got - ref| / max|ref| over everything the solve owns.  NaN or inf on either side gives inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.ndim == 2:
        got, ref = got[None], ref[None]
    with np.errstate(all="ignore"):
        e = np.abs(got - ref).max(axis=(0, 2)) / np.abs(ref).max(axis=(0, 2))
    bad = ~(np.isfinite(got).all(axis=(0, 2)) & np.isfinite(ref).all(axis=(0, 2)))
    return np.where(bad | ~np.isfinite(e), np.inf, e)
