"""Linearised rollout (trajectory + per-step dynamics Jacobians fx, fu) without a GPU: the NumPy helper, discrete_jacobians, and the generated kernel + C ABI +
ctypes binding under the CPU emulation (tests/emu_harness.py).

Reference: tests/rollout_linearized_reference.py - rollout_reference.oracle_rollout for the states; Oracle.fd_grad(..., full=True) for the Jacobians, evaluated at
the state the code under test returned (traj[t, k] cast to fp64) with u[t, k].  Bars: states per solve max|d| / max(1, max|ref|) <= 1e-4 (fp32) / 1e-9 (fp64);
Jacobians per record max|got - ref| <= 1e-4 max|ref| (fp32) / 1e-9 (fp64), fx and fu each on their own, every solve and step, NaN / inf fails.
Inputs: rollout_reference.inputs (q0, qd0 ~ U(-1, 1), u ~ U(-5, 5)), dt = 1e-3, T = 12, N = 5, all eight fixtures.

Room under the bar at these inputs (seed 3), from the reference alone - Oracle(robot, np.float32) against the fp64 oracle on all 60 records of the fp64 oracle
trajectories, worst per-record fx / fu: iiwa14 6.9e-7 / 1.2e-7, hyq 5.1e-7 / 1.4e-7, atlas 6.2e-7 / 1.3e-7, mixed5 3.3e-7 / 1.7e-7, arm6 6.4e-7 / 7.1e-8,
chain12 9.9e-7 / 9.3e-8, chain8 1.1e-6 / 1.0e-7, tree12 1.3e-6 / 1.7e-7: at least 75x inside 1e-4.

Check 3 (what a user does today): under the emulation fx[t] is bit-identical to forward_dynamics_gradient_host at (traj[t], u[t]) on every fixture - the step calls
the same forward_dynamics_gradient_device with the same arguments (the extra qdd / M^-1 outputs of the tip-frame inner do not touch the gradient's arithmetic) -
and that is asserted.  fu against direct_minv_host is bit-identical where the step calls direct_minv_device (atlas, tree12, chain12) and where the column walk
leaves the same M^-1 (mixed5); on the tip-frame robots M^-1 comes from the register factors of the gradient pass, not from direct_minv's own factorisation, and
agrees to rounding (held to the bar).  States against rollout (ABA) agree to rounding, not bit for bit: q̈ comes from the factorisation of M.

Check 4 (discrete Jacobians, no oracle): A, B = discrete_jacobians(fx64, fu64, dt) against central differences (h = 1e-6) of the library's own one-step map
rollout_host_f64(..., final_only=True), T = 1.  Tolerance = 10x the oracle-only figure measured on the same states (inputs(n, 6, 1, 41, float64); A, B built from
Oracle.fd_grad by the block formula against central differences of the oracle's own step), max|d| absolute over all columns of A / B:
iiwa14 8.6e-10 / 4.1e-10, hyq 9.4e-11 / 5.5e-11, chain8 1.5e-10 / 8.5e-11, tree12 1.2e-8 / 4.5e-9, mixed5 B 5.4e-11 (mixed5 A: 5.2e-2 - the reference's first-order
defect for non-root prismatic joints, DESIGN.md sections 2b / 4; robots with such joints are left out of the A check).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from emu_harness import emu_library
from gridcodegenerator_amd import GRiDCodeGenerator, RobotModel
from gridcodegenerator_amd.runtime import discrete_jacobians
from rollout_linearized_reference import JTOL32, JTOL64, block_jacobians, oracle_jacobians, per_record_err
from rollout_reference import FIXTURES, TOL32, TOL64, inputs, oracle_rollout, per_solve_err
from test_generated_emulation import _random_tree_description

HIP_ERROR_INVALID_VALUE = 1  # (value of the emulated hipErrorInvalidValue)
N, T, DT = 5, 12, 1e-3  # N is not a multiple of the solves per wave of any robot
FD_TOL = {"iiwa14": (8.6e-9, 4.1e-9), "hyq": (9.4e-10, 5.5e-10), "chain8": (1.5e-9, 8.5e-10), "tree12": (1.2e-7, 4.5e-8), "mixed5": (None, 5.4e-10)}  # 10x the oracle-only figures (docstring)


@pytest.fixture(scope="module")
def libs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = emu_library(name, max_timesteps=512)
        return cache[name]

    yield get
    for lib in cache.values():
        lib.close()


def check_jacobians(tag, traj, u, fx, fu, name, tol):
    rfx, rfu = oracle_jacobians(name, traj, u)
    efx, efu = per_record_err(fx, rfx), per_record_err(fu, rfu)
    print("[rollout_linearized parity] %s: fx worst %.3g, fu worst %.3g over %d records" % (tag, efx.max(), efu.max(), efx.size))
    assert efx.max() <= tol, (tag, "fx", efx.max())
    assert efu.max() <= tol, (tag, "fu", efu.max())


# ---------------------------------------------------------------------------------------------------- the NumPy statement and the block formula
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5"])
def test_numpy_helper_matches_the_oracle(name):
    robot = RobotModel.from_fixture(name)
    gen = GRiDCodeGenerator(robot)
    n = robot.n
    x0, u = inputs(n, 2, 6, 11, np.float64)
    ref = oracle_rollout(robot, x0, u, DT)
    for k in range(2):
        traj, fx, fu = gen.test_rollout_linearized(x0[k, :n], x0[k, n:], u[:, k], DT)
        assert traj.shape == (7, 2 * n) and fx.shape == (6, 2 * n * n) and fu.shape == (6, n * n)
        assert np.abs(traj - ref[:, k]).max() <= 1e-9
        rfx, rfu = oracle_jacobians(robot, traj[:, None, :], u[:, k:k + 1])
        assert per_record_err(fx[:, None], rfx).max() <= 1e-9 and per_record_err(fu[:, None], rfu).max() <= 1e-9
        F = fu.reshape(6, n, n)
        assert np.array_equal(F, F.swapaxes(-1, -2))


def test_discrete_jacobians_is_the_block_formula():
    import torch

    rng = np.random.default_rng(5)
    n, dt = 4, 0.01
    fx, fu = rng.normal(size=(3, 2, 2 * n * n)), rng.normal(size=(3, 2, n * n))
    A, B = discrete_jacobians(fx, fu, dt)
    assert isinstance(A, np.ndarray) and A.shape == (3, 2, 2 * n, 2 * n) and B.shape == (3, 2, 2 * n, n)
    for t in range(3):
        for k in range(2):
            Ar, Br = block_jacobians(fx[t, k], fu[t, k], dt)
            assert np.allclose(A[t, k], Ar, rtol=1e-15, atol=1e-15) and np.allclose(B[t, k], Br, rtol=1e-15, atol=1e-15)
    # one hand-written entry of every block: d q_{t+1, r} / d qd_{t, c} = dt (delta + dt Fv[r, c]) with Fv[r, c] = fx[(n + c)*n + r]
    r, c = 1, 3
    assert A[0, 0, r, n + c] == dt * (dt * fx[0, 0, (n + c) * n + r])
    assert A[0, 0, n + r, c] == dt * fx[0, 0, c * n + r]
    assert B[0, 0, n + r, c] == dt * fu[0, 0, c * n + r] and B[0, 0, r, c] == dt * dt * fu[0, 0, c * n + r]
    At, Bt = discrete_jacobians(torch.from_numpy(fx), torch.from_numpy(fu), dt)
    assert isinstance(At, torch.Tensor) and At.device == torch.from_numpy(fx).device
    assert np.allclose(At.numpy(), A, rtol=1e-15, atol=1e-15) and np.allclose(Bt.numpy(), B, rtol=1e-15, atol=1e-15)
    A1, B1 = discrete_jacobians(fx[0, 0], fu[0, 0], dt)  # no leading dimensions
    assert np.array_equal(A1, A[0, 0]) and np.array_equal(B1, B[0, 0])
    with pytest.raises(ValueError):
        discrete_jacobians(fx[..., :-1], fu, dt)


# ---------------------------------------------------------------------------------------------------- 1 + 2. every fixture against the oracle
@pytest.mark.parametrize("name", FIXTURES)
def test_emulated_rollout_linearized_matches_the_oracle(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 3)
    traj, fx, fu = lib.rollout_linearized_host(x0, u, DT)
    assert traj.shape == (T + 1, N, 2 * n) and fx.shape == (T, N, 2 * n * n) and fu.shape == (T, N, n * n)
    assert traj.dtype == fx.dtype == fu.dtype == np.float32
    err = per_solve_err(traj, oracle_rollout(name, x0, u, DT))
    print("[rollout_linearized parity] %s fp32 states: worst %.3g" % (name, err.max()))
    assert err.max() <= TOL32
    check_jacobians(name + " fp32", traj, u, fx, fu, name, JTOL32)
    assert np.array_equal(traj[0], x0)
    F = fu.reshape(T, N, n, n)
    assert np.array_equal(F, F.swapaxes(-1, -2))
    # fp64 twin
    x64, u64 = x0.astype(np.float64), u.astype(np.float64)
    t64, fx64, fu64 = lib.rollout_linearized_host_f64(x64, u64, DT)
    assert t64.dtype == fx64.dtype == fu64.dtype == np.float64
    assert per_solve_err(t64, oracle_rollout(name, x64, u64, DT)).max() <= TOL64
    check_jacobians(name + " fp64", t64, u64, fx64, fu64, name, JTOL64)
    assert np.array_equal(t64[0], x64)
    F = fu64.reshape(T, N, n, n)
    assert np.array_equal(F, F.swapaxes(-1, -2))


# ---------------------------------------------------------------------------------------------------- 3. what a user does today
@pytest.mark.parametrize("name", FIXTURES)
def test_agrees_with_the_stepwise_entry_points(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 6)
    traj, fx, fu = lib.rollout_linearized_host(x0, u, DT)
    assert per_solve_err(traj, lib.rollout_host(x0, u, DT).astype(np.float64)).max() <= TOL32
    iu = np.triu_indices(n)
    for t in range(T):
        x = np.hstack([traj[t], u[t]])
        grad = lib.forward_dynamics_gradient_host(x)
        assert np.array_equal(fx[t], grad), (name, t, np.abs(fx[t] - grad).max())  # the same device function with the same arguments
        minv = lib.direct_minv_host(x).reshape(N, n, n)  # [col, row], upper triangle (row <= col)
        got = fu[t].reshape(N, n, n)
        a, b = got[:, iu[1], iu[0]], minv[:, iu[1], iu[0]]
        assert np.isfinite(a).all() and (np.abs(a - b).max(axis=1) <= JTOL32 * np.abs(b).max(axis=1)).all(), (name, t)


# ---------------------------------------------------------------------------------------------------- 4. discrete Jacobians from the library's outputs alone
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "chain8", "tree12", "mixed5"])
def test_discrete_jacobians_against_central_differences_of_the_own_step(name, libs):
    lib = libs(name)
    n = lib.n
    K, h = 6, 1e-6
    x0, u = inputs(n, K, 1, 41, np.float64)
    _, fx, fu = lib.rollout_linearized_host_f64(x0, u, DT)
    A, B = discrete_jacobians(fx[0], fu[0], DT)
    assert A.shape == (K, 2 * n, 2 * n) and B.shape == (K, 2 * n, n)
    # every perturbed state and control of every solve in ONE batch: solve k, column c, sign s
    xs, us = [], []
    for k in range(K):
        for c in range(3 * n):
            for s in (1.0, -1.0):
                x, v = x0[k].copy(), u[0, k].copy()
                if c < 2 * n:
                    x[c] += s * h
                else:
                    v[c - 2 * n] += s * h
                xs.append(x)
                us.append(v)
    out = lib.rollout_host_f64(np.array(xs), np.array(us)[None], DT, final_only=True).reshape(K, 3 * n, 2, 2 * n)
    fd = (out[:, :, 0] - out[:, :, 1]) / (2 * h)  # (K, column, row)
    fdA, fdB = fd[:, :2 * n].swapaxes(1, 2), fd[:, 2 * n:].swapaxes(1, 2)
    eA, eB = np.abs(fdA - A).max(), np.abs(fdB - B).max()
    print("[rollout_linearized layout] %s: max|A - fd| %.3g, max|B - fd| %.3g" % (name, eA, eB))
    tolA, tolB = FD_TOL[name]
    assert eB <= tolB
    if tolA is not None:  # (robots with non-root prismatic joints: fx follows the oracle, whose d/dq is not the derivative there - see the docstring)
        assert eA <= tolA


# ---------------------------------------------------------------------------------------------------- 5. composition
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5", "tree12"])
def test_rollout_linearized_composes(name, libs):
    """12 steps in one call == 5 steps, then 7 more from its xT: states, fx rows and fu rows bit for bit"""
    lib = libs(name)
    x0, u = inputs(lib.n, N, T, 5)
    traj, fx, fu = lib.rollout_linearized_host(x0, u, DT)
    t1, xT, fx1, fu1 = lib.rollout_linearized_host(x0, u[:5], DT, want=("traj", "xT", "fx", "fu"))
    assert np.array_equal(t1, traj[:6]) and np.array_equal(xT, traj[5]) and np.array_equal(fx1, fx[:5]) and np.array_equal(fu1, fu[:5])
    t2, fx2, fu2 = lib.rollout_linearized_host(xT, u[5:], DT)
    assert np.array_equal(t2, traj[5:]) and np.array_equal(fx2, fx[5:]) and np.array_equal(fu2, fu[5:])


# ---------------------------------------------------------------------------------------------------- 6. modes and layouts
@pytest.mark.parametrize("name", ["iiwa14", "atlas", "mixed5", "chain12"])
def test_every_output_mode_gives_the_same_records(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 7)
    traj, xT, fx, fu = lib.rollout_linearized_host(x0, u, DT, want=("traj", "xT", "fx", "fu"))
    assert np.array_equal(xT, traj[T])
    for want, ref in ((("fx",), (fx,)), (("fu",), (fu,)), (("traj",), (traj,)), (("xT",), (xT,)), (("xT", "fu"), (xT, fu)), (("traj", "fx"), (traj, fx))):
        got = lib.rollout_linearized_host(x0, u, DT, want=want)
        assert len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref)), want
    shared = np.ascontiguousarray(u[:, 0])
    dense = lib.rollout_linearized_host(x0, np.ascontiguousarray(np.repeat(shared[:, None, :], N, axis=1)), DT)
    assert all(np.array_equal(a, b) for a, b in zip(lib.rollout_linearized_host(x0, shared, DT), dense))
    wide = np.hstack([x0, np.full((N, n), 1e9, np.float32)])  # (N, 3n): the third block is not read
    assert all(np.array_equal(a, b) for a, b in zip(lib.rollout_linearized_host(wide, shared, DT), dense))
    with pytest.raises(ValueError):
        lib.rollout_linearized_host(x0, u[:, :3], DT)
    with pytest.raises(ValueError):
        lib.rollout_linearized_host(x0[:, :n], u, DT)


# ---------------------------------------------------------------------------------------------------- 7. one diverging solve stays alone
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "tree12"])
def test_a_diverging_solve_does_not_poison_its_neighbours(name, libs):
    lib = libs(name)
    x0, u = inputs(lib.n, N, T, 13)
    clean = lib.rollout_linearized_host(x0, u, DT)
    u_bad = u.copy()
    u_bad[:, 2] = 1e30
    with np.errstate(all="ignore"):
        bad = lib.rollout_linearized_host(x0, u_bad, DT)
    assert not np.isfinite(bad[0][T, 2]).all()  # plain floating point: inf / NaN, nothing faults
    others = [0, 1, 3, 4]
    for a, b in zip(bad, clean):
        assert np.array_equal(a[:, others], b[:, others])


# ---------------------------------------------------------------------------------------------------- 8. boundary behaviour through ctypes
def test_capi_boundary(libs):
    lib = libs("iiwa14")
    L, h, n = lib.lib, lib.handle, lib.n
    x0, u = inputs(n, N, T, 8)
    traj, xT = np.zeros((T + 1, N, 2 * n), np.float32), np.zeros((N, 2 * n), np.float32)
    fx, fu = np.zeros((T, N, 2 * n * n), np.float32), np.zeros((T, N, n * n), np.float32)
    P = lambda a: ctypes.c_void_p(None) if a is None else ctypes.c_void_p(a.ctypes.data)
    f = ctypes.c_float

    def call(fn, x=x0, sx=2 * n, uu=u, sstep=N * n, ssolve=n, nn=N, tt=T, tr=traj, xt=xT, jx=fx, ju=fu):
        a = [h, P(x), sx, P(uu), ctypes.c_long(sstep), ssolve, nn, tt, f(DT), f(9.81), P(tr), P(xt), P(jx), P(ju)]
        return fn(*(a + [ctypes.c_void_p(None)] if fn is L.grid_rollout_linearized_device else a))

    ref = lib.rollout_linearized_host(x0, u, DT, want=("traj", "xT", "fx", "fu"))
    for fn in (L.grid_rollout_linearized_host, L.grid_rollout_linearized_device):  # (under the emulation device memory is host memory)
        for a in (traj, xT, fx, fu):
            a[:] = 0
        assert call(fn) == 0
        assert all(np.array_equal(a, b) for a, b in zip((traj, xT, fx, fu), ref))
        # T = 0 is legal: x0 goes to traj / xT, u is not read, no Jacobian is written
        for a in (traj, xT, fx, fu):
            a[:] = 0
        assert call(fn, tt=0, uu=None) == 0
        assert np.array_equal(traj[0], x0) and np.array_equal(xT, x0) and not traj[1:].any() and not fx.any() and not fu.any()
        assert call(fn, tt=0, uu=None, tr=None, xt=None) == 0 and not fx.any() and not fu.any()
        assert call(fn, nn=0) == 0
        for kw, word in (({"tr": None, "xt": None, "jx": None, "ju": None}, "output"), ({"x": None}, "null"), ({"uu": None}, "null"), ({"nn": -1}, "negative"),
                         ({"tt": -1}, "negative"), ({"sx": 2 * n - 1}, "stride_x0"), ({"ssolve": n - 1}, "stride_u_solve"), ({"ssolve": -n}, "stride_u_solve"),
                         ({"sstep": N * n - 1}, "stride_u_step"), ({"sstep": -N * n}, "stride_u_step"), ({"ssolve": 0, "sstep": n - 1}, "stride_u_step")):
            assert call(fn, **kw) == HIP_ERROR_INVALID_VALUE, kw
            assert word in L.grid_last_error().decode(), (kw, L.grid_last_error().decode())
        for kw in ({"tr": None}, {"xt": None}, {"jx": None}, {"ju": None}, {"tr": None, "xt": None, "ju": None}, {"tr": None, "xt": None, "jx": None}):
            assert call(fn, **kw) == 0, kw
    assert call(lambda *a: L.grid_rollout_linearized_host(None, *a[1:])) == HIP_ERROR_INVALID_VALUE
    assert call(L.grid_rollout_linearized_host, x=np.zeros((N, 4 * n), np.float32), sx=4 * n) == HIP_ERROR_INVALID_VALUE  # host rows: [2n, 3n]
    with pytest.raises(Exception):
        lib.rollout_linearized_host(np.zeros((lib.max_timesteps + 1, 2 * n), np.float32), np.zeros((1, n), np.float32), DT)  # more solves than grid_init's max_timesteps
    # over the documented staging cap of the host form (1 GiB per staged output): refused before anything is allocated, copied or written
    steps = (1 << 30) // (4 * 2 * n * n * N) + 1
    shared = np.zeros((steps, n), np.float32)
    fx[:] = 0
    assert call(L.grid_rollout_linearized_host, uu=shared, sstep=n, ssolve=0, tt=steps, tr=None, xt=None, ju=None) == HIP_ERROR_INVALID_VALUE
    assert "capacity" in L.grid_last_error().decode() and not fx.any()
    # ... and the handle still works, and a longer call than before grows the staging
    x1, u1 = inputs(n, 7, 20, 9)
    t1, fx1, fu1 = lib.rollout_linearized_host(x1, u1, DT)
    assert per_solve_err(t1, oracle_rollout("iiwa14", x1, u1, DT)).max() <= TOL32
    check_jacobians("iiwa14 after the refused call", t1, u1, fx1, fu1, "iiwa14", JTOL32)


# ---------------------------------------------------------------------------------------------------- 9. generator API
def _rnd_prismatic():
    desc = _random_tree_description(13, 7)
    for j in (1, 4, 6):
        desc["joints"][j]["type"] = "prismatic"
    desc["name"] += "p"
    return RobotModel(desc)


@pytest.mark.parametrize("robot", ["iiwa14", "tree12", "prismatic"])
def test_generator_emits_the_rollout_linearized_surface(robot, tmp_path):
    from gridcodegenerator_amd.runtime import generate_header

    model = _rnd_prismatic() if robot == "prismatic" else RobotModel.from_fixture(robot)
    text = open(generate_header(model, str(tmp_path / "a"))).read()
    for decl in ("void rollout_linearized_device(", "void rollout_linearized_kernel(", "void rollout_linearized_kernel_single_timing(", "void rollout_linearized(",
                 "void rollout_linearized_single_timing(", "void rollout_linearized_compute_only(", "void rollout_linearized_reserve("):
        assert text.count(decl) == 1, decl
    for const in ("ROLLOUT_LIN_SUGGESTED_THREADS", "ROLLOUT_LIN_LDS_PER_SOLVE", "ROLLOUT_LIN_OUT_PER_SOLVE", "ROLLOUT_LIN_DYNAMIC_SHARED_MEM_COUNT"):
        assert "const int %s = " % const in text, const
    for member in ("T *d_fx_traj;", "T *h_fx_traj;", "T *d_fu_traj;", "T *h_fu_traj;"):
        assert text.count(member) == text.count("T *d_x_traj;") >= 1, member  # (once per gridData struct: robots with a nested `wide` library declare it twice)
    assert text.count("hd_data->d_fx_traj = nullptr;") == 2 and text.count("hd_data->h_fu_traj = nullptr;") == 2  # (both init_gridData overloads)
    assert text.index("void rollout_reserve(") < text.index("void rollout_linearized_device(")  # after the rollout block
    body = text[text.index("void rollout_linearized_kernel("):text.index("void rollout_linearized_reserve(")]
    assert body.count("rollout_linearized_device<T>(") == 1  # a runtime step loop around one copy of the step
    lines = [ln.strip() for ln in body.splitlines()]
    at = [i for i, ln in enumerate(lines) if ln.startswith("for (int t = 0; t < NUM_STEPS; t++)")]
    assert len(at) == 1 and not lines[at[0] - 1].startswith("#pragma unroll")  # (a runtime loop, not unrolled)
    call = next(i for i, ln in enumerate(lines) if "rollout_linearized_device<T>(" in ln)
    assert at[0] < call
    assert text.count("qd + dt*qdd") == 1  # the update is still written once: the step calls grid_symplectic_euler_step
    assert open(generate_header(model, str(tmp_path / "b"))).read() == text  # deterministic


def test_prismatic_tree_rolls_out_linearized():
    robot = _rnd_prismatic()
    lib = emu_library(robot)
    x0, u = inputs(robot.n, 3, 6, 12)
    traj, fx, fu = lib.rollout_linearized_host(x0, u, DT)
    assert per_solve_err(traj, oracle_rollout(robot, x0, u, DT)).max() <= TOL32
    check_jacobians("random prismatic tree", traj, u, fx, fu, robot, JTOL32)
    lib.close()


# ---------------------------------------------------------------------------------------------------- 10. the emitted host wrappers
def test_generated_host_wrappers_under_emulation(tmp_path):
    """tests/cpp/host_api_rollout_linearized_demo.hip compiled against the emulation: the emitted host wrappers give what the C ABI gives"""
    from gridcodegenerator_amd.runtime import generate_header

    here = os.path.dirname(os.path.abspath(__file__))
    name, n, Nd, S = "iiwa14", 7, 11, 6
    generate_header(RobotModel.from_fixture(name), str(tmp_path / "gen"))
    exe = str(tmp_path / "demo")
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-pthread", "-I" + os.path.join(here, "emu"), "-I" + str(tmp_path / "gen"), "-x", "c++",
                           os.path.join(here, "cpp", "host_api_rollout_linearized_demo.hip"), "-o", exe])
    x0, u = inputs(n, Nd, S, 14)
    (tmp_path / "x0.bin").write_bytes(np.hstack([x0, np.zeros((Nd, n), np.float32)]).astype(np.float64).tobytes())
    (tmp_path / "u.bin").write_bytes(u.astype(np.float64).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "x0.bin"), str(tmp_path / "u.bin"), str(Nd), str(S), repr(DT), str(tmp_path / "f32.bin"), str(tmp_path / "f64.bin")],
                                  text=True, timeout=600)
    assert out.count("Single Call ROLLOUT_LIN") == 2
    assert out.count("max|delta|") == 4
    for line in out.splitlines():
        if "max|delta|" in line:
            assert float(line.split("=")[-1]) == 0.0, line
    lib = emu_library(name)
    for fname, dtype, fn in (("f32.bin", np.float32, lib.rollout_linearized_host), ("f64.bin", np.float64, lib.rollout_linearized_host_f64)):
        got = np.frombuffer((tmp_path / fname).read_bytes(), dtype=np.float64)
        ref = np.concatenate([a.astype(np.float64).reshape(-1) for a in fn(x0.astype(dtype), u.astype(dtype), DT)])
        assert got.shape == ref.shape and np.abs(got - ref).max() == 0.0, fname
    lib.close()
