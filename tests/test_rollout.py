"""Fused multi-step rollout (ABA + semi-implicit Euler) without a GPU: the NumPy helper, and the generated kernel + C ABI + ctypes binding under the
CPU emulation (tests/emu_harness.py).

The reference of every comparison is tests/rollout_reference.py: the fp64 oracle stepped in NumPy fp64, not the code under test.
Error metric: per solve max|got - ref| / max(1, max|ref|); bar 1e-4 (the project's acceptance for fp32 kernels).  With q0, qd0 ~ U(-1, 1),
u ~ U(-5, 5), dt = 1e-3 the fp32 oracle alone stays below 1e-6 of the fp64 one over 64 steps, so the horizon does not amplify rounding.
"""
import ctypes

import numpy as np
import pytest

from emu_harness import emu_library
from gridcodegenerator_amd import GRiDCodeGenerator, RobotModel
from gridcodegenerator_amd.runtime import GridError
from rollout_reference import FIXTURES, TOL32, TOL64, inputs, oracle_rollout, per_solve_err
from test_generated_emulation import _random_tree_description

HIP_ERROR_INVALID_VALUE = 1  # (value of the emulated hipErrorInvalidValue)
N, T, DT = 5, 12, 1e-3  # N is not a multiple of the solves per wave of any robot


@pytest.fixture(scope="module")
def libs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = emu_library(name)
        return cache[name]

    yield get
    for lib in cache.values():
        lib.close()


# ---------------------------------------------------------------------------------------------------- 1. the NumPy statement of the semantics
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5"])
def test_numpy_helper_matches_the_oracle_rollout(name):
    robot = RobotModel.from_fixture(name)
    gen = GRiDCodeGenerator(robot)
    n = robot.n
    x0, u = inputs(n, 2, 16, 11, np.float64)
    ref = oracle_rollout(robot, x0, u, DT)
    for k in range(2):
        got = gen.test_rollout(x0[k, :n], x0[k, n:], u[:, k], DT)
        assert got.shape == (17, 2 * n)
        assert np.array_equal(got[0], x0[k])
        assert np.abs(got - ref[:, k]).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------- 2. every fixture against the oracle rollout
@pytest.mark.parametrize("name", FIXTURES)
def test_emulated_rollout_matches_the_oracle(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 3)
    ref = oracle_rollout(name, x0, u, DT)
    traj = lib.rollout_host(x0, u, DT)
    assert traj.shape == (T + 1, N, 2 * n) and traj.dtype == np.float32
    for t in range(T + 1):  # every row of every solve
        err = per_solve_err(traj[t], ref[t])
        print("%s step %d: worst per-solve error %.3g" % (name, t, err.max()))
        assert err.max() <= TOL32, (name, t, err)
    assert np.array_equal(traj[0], x0)
    xT = lib.rollout_host(x0, u, DT, final_only=True)
    assert xT.shape == (N, 2 * n)
    assert np.array_equal(xT, traj[T])
    # both outputs of one call
    both_traj, both_xT = np.empty_like(traj), np.empty_like(xT)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.lib.grid_rollout_host(lib.handle, P(x0), 2 * n, P(u), ctypes.c_long(N * n), n, N, T, ctypes.c_float(DT), ctypes.c_float(9.81), P(both_traj), P(both_xT)) == 0
    assert np.array_equal(both_traj, traj) and np.array_equal(both_xT, xT)


@pytest.mark.parametrize("name", ["iiwa14", "atlas"])
def test_emulated_rollout_f64(name, libs):
    lib = libs(name)
    x0, u = inputs(lib.n, N, T, 4, np.float64)
    traj = lib.rollout_host_f64(x0, u, DT)
    assert traj.dtype == np.float64
    assert per_solve_err(traj, oracle_rollout(name, x0, u, DT)).max() <= TOL64
    assert np.array_equal(lib.rollout_host_f64(x0, u, DT, final_only=True), traj[T])


# ---------------------------------------------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5"])
def test_rollout_composes(name, libs):
    """The state never leaves fp32: 12 steps == 5 steps, then 7 more from its xT, bit for bit"""
    lib = libs(name)
    x0, u = inputs(lib.n, N, T, 5)
    whole = lib.rollout_host(x0, u, DT)
    first = lib.rollout_host(x0, u[:5], DT, final_only=True)
    assert np.array_equal(first, whole[5])
    second = lib.rollout_host(first, u[5:], DT)
    assert np.array_equal(second, whole[5:])


# ---------------------------------------------------------------------------------------------------- 4. what a user does today
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5"])
def test_rollout_equals_stepwise_aba(name, libs):
    """T calls of the existing aba entry point with the update in NumPy float32: the same arithmetic (no FMA contraction under the emulation)"""
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 6)
    traj = lib.rollout_host(x0, u, DT)
    q, qd = x0[:, :n].copy(), x0[:, n:].copy()
    dt = np.float32(DT)
    for t in range(T):
        qdd = lib.forward_dynamics_host(np.hstack([q, qd, u[t]]), aba=True)
        assert qdd.dtype == np.float32
        qd = qd + dt * qdd
        q = q + dt * qd
        assert q.dtype == np.float32
        assert np.array_equal(traj[t + 1], np.hstack([q, qd])), (name, t)


# ---------------------------------------------------------------------------------------------------- 5. layouts
@pytest.mark.parametrize("name", ["iiwa14", "tree12"])
def test_shared_control_and_wide_x0_rows(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 7)
    shared = np.ascontiguousarray(u[:, 0])
    dense = lib.rollout_host(x0, np.ascontiguousarray(np.repeat(shared[:, None, :], N, axis=1)), DT)
    assert np.array_equal(lib.rollout_host(x0, shared, DT), dense)
    wide = np.hstack([x0, np.full((N, n), 1e9, np.float32)])  # (N, 3n): the third block is not read
    assert np.array_equal(lib.rollout_host(wide, shared, DT), dense)
    with pytest.raises(ValueError):
        lib.rollout_host(x0, u[:, :3], DT)
    with pytest.raises(ValueError):
        lib.rollout_host(x0[:, :n], u, DT)


# ---------------------------------------------------------------------------------------------------- 6. boundary behaviour through ctypes
def test_capi_boundary(libs):
    lib = libs("iiwa14")
    L, h, n = lib.lib, lib.handle, lib.n
    x0, u = inputs(n, N, T, 8)
    traj, xT = np.zeros((T + 1, N, 2 * n), np.float32), np.zeros((N, 2 * n), np.float32)
    P = lambda a: ctypes.c_void_p(None) if a is None else ctypes.c_void_p(a.ctypes.data)
    f = ctypes.c_float

    def call(fn, x=x0, sx=2 * n, uu=u, sstep=N * n, ssolve=n, nn=N, tt=T, tr=traj, xt=xT):
        a = [h, P(x), sx, P(uu), ctypes.c_long(sstep), ssolve, nn, tt, f(DT), f(9.81), P(tr), P(xt)]
        return fn(*(a + [ctypes.c_void_p(None)] if fn is L.grid_rollout_device else a))

    for fn in (L.grid_rollout_host, L.grid_rollout_device):  # (under the emulation device memory is host memory)
        assert call(fn) == 0
        assert np.array_equal(traj[T], xT)
        # T = 0 is legal: x0 goes to the outputs, u is not read
        traj[:] = xT[:] = 0
        assert call(fn, tt=0, uu=None) == 0
        assert np.array_equal(traj[0], x0) and np.array_equal(xT, x0) and not traj[1:].any()
        assert call(fn, nn=0) == 0
        for kw, word in (({"tr": None, "xt": None}, "output"), ({"x": None}, "null"), ({"uu": None}, "null"), ({"nn": -1}, "negative"), ({"tt": -1}, "negative"),
                         ({"sx": 2 * n - 1}, "stride_x0"), ({"ssolve": n - 1}, "stride_u_solve"), ({"ssolve": -n}, "stride_u_solve"),
                         ({"sstep": N * n - 1}, "stride_u_step"), ({"sstep": -N * n}, "stride_u_step"), ({"ssolve": 0, "sstep": n - 1}, "stride_u_step")):
            assert call(fn, **kw) == HIP_ERROR_INVALID_VALUE, kw
            assert word in lib.lib.grid_last_error().decode(), (kw, lib.lib.grid_last_error().decode())
        assert call(fn, xt=None) == 0 and call(fn, tr=None) == 0
    assert L.grid_rollout_host(None, P(x0), 2 * n, P(u), ctypes.c_long(N * n), n, N, T, f(DT), f(9.81), P(traj), P(xT)) == HIP_ERROR_INVALID_VALUE
    assert call(L.grid_rollout_host, x=np.zeros((N, 4 * n), np.float32), sx=4 * n) == HIP_ERROR_INVALID_VALUE  # host rows: [2n, 3n]
    big = np.zeros((lib.max_timesteps + 1, 2 * n), np.float32)
    with pytest.raises(GridError):
        lib.rollout_host(big, np.zeros((1, n), np.float32), DT)  # more solves than grid_init's max_timesteps
    # the handle still works, and a longer call grows the staging
    x1, u1 = inputs(n, 7, 20, 9)
    assert per_solve_err(lib.rollout_host(x1, u1, DT), oracle_rollout("iiwa14", x1, u1, DT)).max() <= TOL32


# ---------------------------------------------------------------------------------------------------- 7. generator API
def _rnd_prismatic():
    desc = _random_tree_description(13, 7)
    for j in (1, 4, 6):
        desc["joints"][j]["type"] = "prismatic"
    desc["name"] += "p"
    return RobotModel(desc)


@pytest.mark.parametrize("robot", ["iiwa14", "tree12", "prismatic"])
def test_generator_emits_the_rollout_surface(robot, tmp_path):
    from gridcodegenerator_amd.runtime import generate_header

    text = open(generate_header(_rnd_prismatic() if robot == "prismatic" else RobotModel.from_fixture(robot), str(tmp_path))).read()
    for decl in ("void rollout_device(", "void rollout_kernel(", "void rollout_kernel_single_timing(", "void rollout(", "void rollout_single_timing(",
                 "void rollout_compute_only(", "void rollout_reserve(", "void grid_symplectic_euler_step("):
        assert text.count(decl) == 1, decl
    for const in ("ROLLOUT_SUGGESTED_THREADS", "ROLLOUT_LDS_PER_SOLVE", "ROLLOUT_OUT_PER_SOLVE", "ROLLOUT_DYNAMIC_SHARED_MEM_COUNT"):
        assert "const int %s = " % const in text, const
    body = text[text.index("void rollout_kernel("):text.index("void rollout_reserve(")]
    assert body.count("rollout_device<T>(") == 1  # a runtime step loop around one copy of the inner
    lines = [ln.strip() for ln in body.splitlines()]
    at = [i for i, ln in enumerate(lines) if ln.startswith("for (int t = 0; t < NUM_STEPS; t++)")]
    assert len(at) == 1 and not lines[at[0] - 1].startswith("#pragma unroll")  # (a runtime loop, not unrolled)
    assert text.count("qd + dt*qdd") == 1  # the update is written once


def test_prismatic_tree_rolls_out():
    robot = _rnd_prismatic()
    lib = emu_library(robot)
    x0, u = inputs(robot.n, 3, 6, 12)
    assert per_solve_err(lib.rollout_host(x0, u, DT), oracle_rollout(robot, x0, u, DT)).max() <= TOL32
    lib.close()


def test_generated_host_wrappers_under_emulation(tmp_path):
    """tests/cpp/host_api_rollout_demo.hip (rollout_reserve, rollout, rollout_single_timing, rollout_compute_only, close_grid) compiled against the emulation"""
    import os
    import subprocess

    from gridcodegenerator_amd.runtime import generate_header

    here = os.path.dirname(os.path.abspath(__file__))
    n, Nd, S = 7, 11, 6
    generate_header(RobotModel.from_fixture("iiwa14"), str(tmp_path / "gen"))
    exe = str(tmp_path / "demo")
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-pthread", "-I" + os.path.join(here, "emu"), "-I" + str(tmp_path / "gen"), "-x", "c++",
                           os.path.join(here, "cpp", "host_api_rollout_demo.hip"), "-o", exe])
    x0, u = inputs(n, Nd, S, 14, np.float64)
    (tmp_path / "x0.bin").write_bytes(np.hstack([x0, np.zeros((Nd, n))]).tobytes())
    (tmp_path / "u.bin").write_bytes(u.tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "x0.bin"), str(tmp_path / "u.bin"), str(Nd), str(S), repr(DT), str(tmp_path / "f32.bin"), str(tmp_path / "f64.bin")],
                                  text=True, timeout=600)
    assert out.count("Single Call ROLLOUT") == 2
    for line in out.splitlines():
        if "max|delta|" in line:
            assert float(line.split("=")[-1]) == 0.0, line
    ref = oracle_rollout("iiwa14", x0, u, DT)
    for f, tol in (("f32.bin", TOL32), ("f64.bin", TOL64)):
        got = np.frombuffer((tmp_path / f).read_bytes(), dtype=np.float64).reshape(S + 1, Nd, 2 * n)
        assert per_solve_err(got, ref).max() <= tol


# ---------------------------------------------------------------------------------------------------- 8. one diverging solve stays alone
@pytest.mark.parametrize("name", ["iiwa14", "hyq"])
def test_a_diverging_solve_does_not_poison_its_neighbours(name, libs):
    lib = libs(name)
    x0, u = inputs(lib.n, N, T, 13)
    clean = lib.rollout_host(x0, u, DT)
    u_bad = u.copy()
    u_bad[:, 2] = 1e30
    with np.errstate(all="ignore"):
        bad = lib.rollout_host(x0, u_bad, DT)
    assert not np.isfinite(bad[T, 2]).all()  # plain floating point: inf / NaN, nothing faults
    others = [0, 1, 3, 4]
    assert np.array_equal(bad[:, others], clean[:, others])
