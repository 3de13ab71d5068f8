"""Rollout adjoint (gradient of a trajectory cost with respect to x0 and every u_t) without a GPU: the NumPy helper, the generated kernel + C ABI + ctypes binding
under the CPU emulation (tests/emu_harness.py), and rollout_torch on CPU tensors.

Reference: tests/rollout_adjoint_reference.py - A_t, B_t from rollout_linearized_reference.block_jacobians of the fp64 oracle's Jacobians at the traj and u handed to
the code under test, then the un-collapsed recurrence lam_t = g_t + A_t^T lam_{t+1}, grad_u_t = B_t^T lam_{t+1} in fp64.  Error per solve: max|d| / max|ref| over
the solve's grad_x0 record and over all (t, j) of its grad_u, each on its own; NaN / inf fails.  Bars: 1e-4 (fp32), 1e-9 (fp64).
Inputs: rollout_reference.inputs (q0, qd0 ~ U(-1, 1), u ~ U(-5, 5)), g ~ U(-1, 1) at every step, dt = 1e-3, N = 11 (two waves on every robot, not a multiple of
any robot's solves per wave), T = 5, all eight fixtures.

Check 4 (finite differences, no oracle): the directional derivative <grad_x0, dx> + sum_t <grad_u_t, du_t> of the fp64 adjoint against the central difference
(h = 1e-6) of L = sum traj*g under the library's own rollout_host_f64, K = 6 solves, T = 16, one random direction per solve, rel = |fd - an| / max(|fd|, |an|).
Tolerance = 10x what the oracle-only recurrence gives on the SAME inputs and directions (oracle_rollout + oracle_adjoint, measured):
iiwa14 6.35e-9, hyq 2.34e-9, chain8 5.22e-9, tree12 7.05e-9 (mixed5: 9.1e-2 - fx follows the oracle, whose d/dq carries the reference's first-order defect for
non-root prismatic joints, DESIGN.md sections 2b / 4 / 6g; robots with such joints are left out, as in test_rollout_linearized.py).

Check 5 (composition): lam passes through memory in the kernel's own precision and the step arithmetic does not depend on where a call starts, so the split pass
is bit-identical to the whole one under the emulation, fp32 and fp64; that is asserted (the fp64 bar of the issue, 1e-12, is implied).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from emu_harness import emu_library
from gridcodegenerator_amd import GRiDCodeGenerator, RobotModel
from gridcodegenerator_amd.runtime import discrete_jacobians
from rollout_adjoint_reference import ATOL32, ATOL64, cotangent, oracle_adjoint, per_solve_err
from rollout_reference import FIXTURES, inputs, oracle_rollout
from test_generated_emulation import _random_tree_description

HIP_ERROR_INVALID_VALUE = 1  # (value of the emulated hipErrorInvalidValue)
N, T, DT = 11, 5, 1e-3
FD_TOL = {"iiwa14": 6.35e-8, "hyq": 2.34e-8, "chain8": 5.22e-8, "tree12": 7.05e-8}  # 10x the oracle-only figures (docstring)


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


def check(tag, name, traj, u, got_x0, got_u, tol, **cot):
    rx0, ru = oracle_adjoint(name, traj, u, DT, **cot)
    ex, eu = per_solve_err(got_x0, rx0), per_solve_err(got_u, ru)
    print("[rollout_adjoint parity] %s: grad_x0 worst %.3g, grad_u worst %.3g over %d solves" % (tag, ex.max(), eu.max(), ex.size))
    assert ex.max() <= tol, (tag, "grad_x0", ex.max())
    assert eu.max() <= tol, (tag, "grad_u", eu.max())


# ---------------------------------------------------------------------------------------------------- 1. the NumPy statement
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5"])
def test_numpy_helper_matches_the_reference(name):
    robot = RobotModel.from_fixture(name)
    gen = GRiDCodeGenerator(robot)
    n = robot.n
    x0, u = inputs(n, 2, 6, 11, np.float64)
    g = cotangent(n, 2, 6, 11, np.float64)
    traj = oracle_rollout(robot, x0, u, DT)
    rx0, ru = oracle_adjoint(robot, traj, u, DT, gx=g)
    for k in range(2):
        gx0, gu = gen.test_rollout_adjoint(traj[:, k], u[:, k], DT, gx=g[:, k])
        assert gx0.shape == (2 * n,) and gu.shape == (6, n)
        assert per_solve_err(gx0[None], rx0[k:k + 1]).max() <= ATOL64 and per_solve_err(gu[:, None], ru[:, k:k + 1]).max() <= ATOL64
        # gxT alone is gx with every row but the last zero; both add at step T
        gT0, gTu = gen.test_rollout_adjoint(traj[:, k], u[:, k], DT, gxT=g[6, k])
        z = np.zeros_like(g[:, k])
        z[6] = g[6, k]
        a0, au = gen.test_rollout_adjoint(traj[:, k], u[:, k], DT, gx=z)
        assert np.array_equal(gT0, a0) and np.array_equal(gTu, au)
        b0, bu = gen.test_rollout_adjoint(traj[:, k], u[:, k], DT, gx=g[:, k], gxT=g[6, k])
        assert np.allclose(b0, gx0 + gT0, rtol=1e-12, atol=1e-12) and np.allclose(bu, gu + gTu, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- 2. every fixture against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_emulated_rollout_adjoint_matches_the_reference(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 3)
    g = cotangent(n, N, T, 3)
    traj = lib.rollout_host(x0, u, DT)
    gx0, gu = lib.rollout_adjoint_host(traj, u, DT, gx=g)
    assert gx0.shape == (N, 2 * n) and gu.shape == (T, N, n) and gx0.dtype == gu.dtype == np.float32
    check(name + " fp32", name, traj, u, gx0, gu, ATOL32, gx=g)
    x64, u64, g64 = x0.astype(np.float64), u.astype(np.float64), g.astype(np.float64)
    t64 = lib.rollout_host_f64(x64, u64, DT)
    a0, au = lib.rollout_adjoint_host_f64(t64, u64, DT, gx=g64)
    assert a0.dtype == au.dtype == np.float64
    check(name + " fp64", name, t64, u64, a0, au, ATOL64, gx=g64)


# ---------------------------------------------------------------------------------------------------- 3. layout from the library alone
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5", "tree12"])
def test_unit_cotangents_give_the_rows_of_the_discrete_jacobians(name, libs):
    """T = 1, gxT = e_i: grad_x0 is row i of A_0 and grad_u row i of B_0 of discrete_jacobians(rollout_linearized_host_f64) - pins [col*n + row], the q / qd order, the dt powers"""
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, 1, 1, 17, np.float64)
    traj, fx, fu = lib.rollout_linearized_host_f64(x0, u, DT)
    A, B = discrete_jacobians(fx[0, 0], fu[0, 0], DT)
    # all 2n unit vectors in one batch of 2n solves at the same state
    trajs = np.ascontiguousarray(np.repeat(traj, 2 * n, axis=1))
    us = np.ascontiguousarray(np.repeat(u, 2 * n, axis=1))
    gx0, gu = lib.rollout_adjoint_host_f64(trajs, us, DT, gxT=np.eye(2 * n))
    assert np.abs(gx0 - A).max() <= 1e-12, np.abs(gx0 - A).max()
    assert np.abs(gu[0] - B).max() <= 1e-12, np.abs(gu[0] - B).max()
    assert np.abs(A - np.eye(2 * n)).max() > 1e-6 and np.abs(B).max() > 1e-6  # (the comparison is not between zeros)


# ---------------------------------------------------------------------------------------------------- 4. finite differences of the library's own rollout
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "chain8", "tree12"])
def test_adjoint_against_central_differences_of_the_own_rollout(name, libs):
    lib = libs(name)
    n = lib.n
    K, S, h = 6, 16, 1e-6
    x0, u = inputs(n, K, S, 41, np.float64)
    g = cotangent(n, K, S, 41, np.float64)
    rng = np.random.default_rng(77)
    dx, du = rng.uniform(-1, 1, x0.shape), rng.uniform(-1, 1, u.shape)
    traj = lib.rollout_host_f64(x0, u, DT)
    gx0, gu = lib.rollout_adjoint_host_f64(traj, u, DT, gx=g)
    an = (gx0 * dx).sum(axis=1) + (gu * du).sum(axis=(0, 2))
    Lp = (lib.rollout_host_f64(x0 + h * dx, u + h * du, DT) * g).sum(axis=(0, 2))
    Lm = (lib.rollout_host_f64(x0 - h * dx, u - h * du, DT) * g).sum(axis=(0, 2))
    fd = (Lp - Lm) / (2 * h)
    rel = np.abs(fd - an) / np.maximum(np.abs(an), np.abs(fd))
    print("[rollout_adjoint fd] %s: worst rel %.3g over %d solves (tolerance %.3g)" % (name, rel.max(), K, FD_TOL[name]))
    assert np.isfinite(rel).all() and rel.max() <= FD_TOL[name]


# ---------------------------------------------------------------------------------------------------- 5. composition
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5", "tree12"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rollout_adjoint_composes(name, dtype, libs):
    """T1 + T2 steps in one call == the last T2 steps, then the first T1 with gxT = lam_{T1} (g at T1 counted once): bit for bit"""
    lib = libs(name)
    n = lib.n
    f64 = dtype == np.float64
    roll, adj = (lib.rollout_host_f64, lib.rollout_adjoint_host_f64) if f64 else (lib.rollout_host, lib.rollout_adjoint_host)
    x0, u = inputs(n, N, T, 5, dtype)
    g = cotangent(n, N, T, 5, dtype)
    traj = roll(x0, u, DT)
    gx0, gu = adj(traj, u, DT, gx=g)
    T1 = 2
    lam, gu2 = adj(np.ascontiguousarray(traj[T1:]), np.ascontiguousarray(u[T1:]), DT, gx=np.ascontiguousarray(g[T1:]))
    g1 = g[:T1 + 1].copy()
    g1[T1] = 0  # (g at T1 is inside lam already)
    b0, gu1 = adj(np.ascontiguousarray(traj[:T1 + 1]), np.ascontiguousarray(u[:T1]), DT, gx=g1, gxT=lam)
    assert np.array_equal(gu2, gu[T1:]) and np.array_equal(gu1, gu[:T1]) and np.array_equal(b0, gx0)
    if f64:
        assert np.abs(b0 - gx0).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------- 6. modes
@pytest.mark.parametrize("name", ["iiwa14", "atlas", "mixed5", "chain12"])
def test_every_mode_gives_the_same_records(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 7)
    g = cotangent(n, N, T, 7)
    traj = lib.rollout_host(x0, u, DT)
    gx0, gu = lib.rollout_adjoint_host(traj, u, DT, gx=g)
    (a0,) = lib.rollout_adjoint_host(traj, u, DT, gx=g, want=("grad_x0",))
    (au,) = lib.rollout_adjoint_host(traj, u, DT, gx=g, want=("grad_u",))
    bu, b0 = lib.rollout_adjoint_host(traj, u, DT, gx=g, want=("grad_u", "grad_x0"))
    assert np.array_equal(a0, gx0) and np.array_equal(au, gu) and np.array_equal(b0, gx0) and np.array_equal(bu, gu)
    # gx only == gx with its last row moved to gxT == half of each
    head = g.copy()
    head[T] = 0
    c0, cu = lib.rollout_adjoint_host(traj, u, DT, gx=head, gxT=g[T])
    assert np.array_equal(c0, gx0) and np.array_equal(cu, gu)
    # gxT only == gx that is zero before the last row
    tail = np.zeros_like(g)
    tail[T] = g[T]
    d0, du = lib.rollout_adjoint_host(traj, u, DT, gxT=g[T])
    e0, eu = lib.rollout_adjoint_host(traj, u, DT, gx=tail)
    assert np.array_equal(d0, e0) and np.array_equal(du, eu)
    check(name + " gxT only", name, traj, u, d0, du, ATOL32, gxT=g[T])
    # one control sequence for all solves == the tiled one; grad_u stays per solve
    shared = np.ascontiguousarray(u[:, 0])
    tiled = np.ascontiguousarray(np.repeat(shared[:, None, :], N, axis=1))
    ts = lib.rollout_host(x0, shared, DT)
    s0, su = lib.rollout_adjoint_host(ts, shared, DT, gx=g)
    t0, tu = lib.rollout_adjoint_host(ts, tiled, DT, gx=g)
    assert su.shape == (T, N, n) and np.array_equal(s0, t0) and np.array_equal(su, tu)
    # T = 0: grad_x0 = gx[0] (+ gxT), no grad_u
    z0, zu = lib.rollout_adjoint_host(traj[:1], u[:0], DT, gx=g[:1], gxT=g[T])
    assert zu.shape == (0, N, n) and np.array_equal(z0, g[0] + g[T])
    (z1,) = lib.rollout_adjoint_host(traj[:1], np.zeros((0, n), np.float32), DT, gx=g[:1], want=("grad_x0",))
    assert np.array_equal(z1, g[0])
    for bad in (dict(gx=g[:T]), dict(gxT=g[T, :3]), dict(gx=g, want=()), dict(gx=g, want=("fx",))):
        with pytest.raises(ValueError):
            lib.rollout_adjoint_host(traj, u, DT, **bad)
    with pytest.raises(ValueError):
        lib.rollout_adjoint_host(traj, u[:, :3], DT, gx=g)
    with pytest.raises(Exception):
        lib.rollout_adjoint_host(traj, u, DT)  # no cotangent at all


# ---------------------------------------------------------------------------------------------------- 7. diverging solves stay alone
@pytest.mark.parametrize("name", ["iiwa14", "hyq", "tree12"])
def test_diverging_solves_do_not_poison_their_neighbours(name, libs):
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 13)
    g = cotangent(n, N, T, 13)
    traj = lib.rollout_host(x0, u, DT)
    clean = lib.rollout_adjoint_host(traj, u, DT, gx=g)
    tb, ub, gb = traj.copy(), u.copy(), g.copy()
    tb[2, 1] = np.nan       # a NaN state in solve 1
    gb[T, 5, 0] = np.inf    # an infinite cotangent in solve 5
    ub[:, 9] = 3e38         # overflowing controls in solve 9
    with np.errstate(all="ignore"):
        bad = lib.rollout_adjoint_host(tb, ub, DT, gx=gb)
    assert not np.isfinite(bad[0][1]).all() and not np.isfinite(bad[0][5]).all()  # plain floating point: inf / NaN, nothing faults
    others = [k for k in range(N) if k not in (1, 5, 9)]
    for a, b in zip(bad, clean):
        assert np.array_equal(a[..., others, :], b[..., others, :])


# ---------------------------------------------------------------------------------------------------- 8. boundary behaviour through ctypes
def test_capi_boundary(libs):
    lib = libs("iiwa14")
    L, h, n = lib.lib, lib.handle, lib.n
    x0, u = inputs(n, N, T, 8)
    g = cotangent(n, N, T, 8)
    traj = lib.rollout_host(x0, u, DT)
    gT = np.ascontiguousarray(g[T])
    o0, ou = np.zeros((N, 2 * n), np.float32), np.zeros((T, N, n), np.float32)
    P = lambda a: ctypes.c_void_p(None) if a is None else ctypes.c_void_p(a.ctypes.data)
    f = ctypes.c_float

    def call(fn, tr=traj, uu=u, sstep=N * n, ssolve=n, nn=N, tt=T, gx=g, gxT=gT, g0=o0, gu=ou):
        a = [h, P(tr), P(uu), ctypes.c_long(sstep), ssolve, nn, tt, f(DT), f(9.81), P(gx), P(gxT), P(g0), P(gu)]
        return fn(*(a + [ctypes.c_void_p(None)] if fn is L.grid_rollout_adjoint_device else a))

    ref = lib.rollout_adjoint_host(traj, u, DT, gx=g, gxT=gT)
    for fn in (L.grid_rollout_adjoint_host, L.grid_rollout_adjoint_device):  # (under the emulation device memory is host memory)
        o0[:], ou[:] = 0, 0
        assert call(fn) == 0
        assert np.array_equal(o0, ref[0]) and np.array_equal(ou, ref[1])
        # T = 0 is legal: grad_x0 = gx[0] + gxT, neither traj nor u is read, no grad_u is written
        o0[:], ou[:] = 0, 0
        assert call(fn, tt=0, tr=None, uu=None) == 0
        assert np.array_equal(o0, g[0] + gT) and not ou.any()
        assert call(fn, tt=0, g0=None) == 0 and not ou.any()
        assert call(fn, nn=0) == 0
        for kw, word in (({"nn": -1}, "negative"), ({"tt": -1}, "negative"), ({"tr": None}, "null"), ({"uu": None}, "null"), ({"gx": None, "gxT": None}, "cotangent"),
                         ({"g0": None, "gu": None}, "output"), ({"ssolve": n - 1}, "stride_u_solve"), ({"ssolve": -n}, "stride_u_solve"),
                         ({"sstep": N * n - 1}, "stride_u_step"), ({"sstep": -N * n}, "stride_u_step"), ({"ssolve": 0, "sstep": n - 1}, "stride_u_step")):
            assert call(fn, **kw) == HIP_ERROR_INVALID_VALUE, kw
            assert word in L.grid_last_error().decode(), (kw, L.grid_last_error().decode())
        for kw in ({"gx": None}, {"gxT": None}, {"g0": None}, {"gu": None}):
            assert call(fn, **kw) == 0, kw
    assert call(lambda *a: L.grid_rollout_adjoint_host(None, *a[1:])) == HIP_ERROR_INVALID_VALUE
    with pytest.raises(Exception):
        lib.rollout_adjoint_host(np.zeros((2, lib.max_timesteps + 1, 2 * n), np.float32), np.zeros((1, n), np.float32), DT, gxT=np.zeros((lib.max_timesteps + 1, 2 * n), np.float32))
    # over the documented staging cap of the host form (1 GiB per staged record): refused before anything is allocated, copied or written.  The call hands over
    # buffers far shorter than it claims: had it been accepted, the first copy would have run off their end
    steps = (1 << 30) // (4 * 2 * n * N) + 1
    o0[:] = 0
    assert call(L.grid_rollout_adjoint_host, sstep=n, ssolve=0, tt=steps, gu=None) == HIP_ERROR_INVALID_VALUE
    assert "capacity" in L.grid_last_error().decode() and not o0.any()
    # ... and the handle still works, and a longer call than before grows the staging
    x1, u1 = inputs(n, 13, 9, 9)
    g1 = cotangent(n, 13, 9, 9)
    t1 = lib.rollout_host(x1, u1, DT)
    a0, au = lib.rollout_adjoint_host(t1, u1, DT, gx=g1)
    check("iiwa14 after the refused call", "iiwa14", t1, u1, a0, au, ATOL32, gx=g1)


# ---------------------------------------------------------------------------------------------------- 9. generator API
def _rnd_prismatic():
    desc = _random_tree_description(13, 7)
    for j in (1, 4, 6):
        desc["joints"][j]["type"] = "prismatic"
    desc["name"] += "p"
    return RobotModel(desc)


PARENT_SURFACE_END = "void rollout_linearized_compute_only("  # the last function the generator emitted before the adjoint block existed


@pytest.mark.parametrize("robot", ["iiwa14", "tree12", "prismatic"])
def test_generator_emits_the_rollout_adjoint_surface(robot, tmp_path):
    from gridcodegenerator_amd.runtime import generate_header

    model = _rnd_prismatic() if robot == "prismatic" else RobotModel.from_fixture(robot)
    text = open(generate_header(model, str(tmp_path / "a"))).read()
    for decl in ("void rollout_linearize_device(", "void rollout_adjoint_contract_device(", "void rollout_adjoint_device(", "void rollout_adjoint_kernel(",
                 "void rollout_adjoint_kernel_single_timing(", "void rollout_adjoint(", "void rollout_adjoint_single_timing(", "void rollout_adjoint_compute_only(",
                 "void rollout_adjoint_reserve("):
        assert text.count(decl) == 1, decl
    for const in ("ROLLOUT_ADJ_SUGGESTED_THREADS", "ROLLOUT_ADJ_LDS_PER_SOLVE", "ROLLOUT_ADJ_OUT_PER_SOLVE", "ROLLOUT_ADJ_OFF_LAM", "ROLLOUT_ADJ_DYNAMIC_SHARED_MEM_COUNT"):
        assert "const int %s = " % const in text, const
    for member in ("T *d_gx_traj;", "T *h_gx_traj;", "T *d_gu_traj;", "T *h_gu_traj;", "T *d_gx0;", "T *h_gx0;"):
        assert text.count(member) == text.count("T *d_x_traj;") >= 1, member  # (once per gridData struct: robots with a nested `wide` library declare it twice)
    assert text.count("hd_data->d_gx_traj = nullptr;") == 2 and text.count("hd_data->h_gx0 = nullptr;") == 2  # (both init_gridData overloads)
    assert text.count("grid_ee_release(&hd_data->d_gx_traj, &hd_data->h_gx_traj);") == 1
    assert text.index(PARENT_SURFACE_END) < text.index("ROLLOUT_ADJ_LDS_PER_SOLVE = ") < text.index("void rollout_linearize_device(")  # after the rollout_linearized block
    body = text[text.index("void rollout_adjoint_kernel("):text.index("void rollout_adjoint_reserve(")]
    lines = [ln.strip() for ln in body.splitlines()]
    at = [i for i, ln in enumerate(lines) if ln.startswith("for (int t = NUM_STEPS - 1; t >= 0; t--)")]
    assert len(at) == 1 and not lines[at[0] - 1].startswith("#pragma unroll")  # (a runtime loop in reverse time, not unrolled)
    assert body.count("rollout_adjoint_device<T>(") + body.count("rollout_linearize_device<T>(") == 1  # around ONE copy of the step
    assert "static_cast<size_t>(t)*gu_stride" in body and "static_cast<size_t>(t - 1)*row_stride" in body  # 64-bit row offsets
    lin = text[text.index("void rollout_linearized_device("):text.index("void rollout_linearized_kernel_single_timing(")]
    assert "rollout_linearize_device" not in lin  # rollout_linearized_device keeps its own text
    assert text.count("qd + dt*qdd") == 1  # the adjoint needs no state update
    assert open(generate_header(model, str(tmp_path / "b"))).read() == text  # deterministic


@pytest.mark.parametrize("robot", ["iiwa14", "tree12", "prismatic"])
def test_the_adjoint_only_adds_whole_lines(robot, tmp_path):
    """No line the generator emitted before this feature is removed or changed: everything that names the adjoint is either inside ONE contiguous block behind the
    rollout_linearized block, or a whole line of its own of one of five kinds (gridData member, null-initialisation, release, struct comment, documentation)"""
    import re
    from gridcodegenerator_amd.runtime import generate_header

    model = _rnd_prismatic() if robot == "prismatic" else RobotModel.from_fixture(robot)
    lines = open(generate_header(model, str(tmp_path / "a"))).read().splitlines()
    words = ("rollout_adjoint", "ROLLOUT_ADJ", "rollout_linearize_device", "gx_traj", "gu_traj", "gx0", "ROLLOUT ADJOINT", "rollout adjoint")
    start = next(i for i, ln in enumerate(lines) if "// rollout_adjoint: T reverse steps" in ln) - 1
    end = next(i for i, ln in enumerate(lines) if "void rollout_adjoint_compute_only(" in ln)
    indent = lines[end][:len(lines[end]) - len(lines[end].lstrip())]
    end = next(i for i in range(end, len(lines)) if lines[i] == indent + "}")  # the closing brace of the last host wrapper
    assert max(i for i, ln in enumerate(lines) if "void rollout_linearized_compute_only(" in ln) < start
    block = lines[start:end + 1]
    assert sum("__global__" in ln for ln in block) == 2 and sum(ln.strip().startswith("void rollout_linearized") for ln in block) == 0
    kinds = [r"^\s*T \*[dh]_(gx_traj|gu_traj|gx0);(\s*T \*[dh]_(gx_traj|gu_traj|gx0);)*$", r"^\s*hd_data->[dh]_(gx_traj|gu_traj|gx0) = nullptr;$",
             r"^\s*grid_ee_release\(&hd_data->d_gx_traj, &hd_data->h_gx_traj\); grid_ee_release\(&hd_data->d_gu_traj, &hd_data->h_gu_traj\); grid_ee_release\(&hd_data->d_gx0, &hd_data->h_gx0\); // .*$",
             r"^\s*// ROLLOUT ADJOINT .*$", r"^\s*(\* |// )?\s*(rollout adjoint, no counterpart|__device__ rollout_linearize_device<T>|__device__ rollout_adjoint_|__global__ rollout_adjoint_kernel<T>|__host__   rollout_adjoint).*$"]
    outside = [ln for ln in lines[:start] + lines[end + 1:] if any(w in ln for w in words)]
    assert outside
    for ln in outside:
        assert any(re.match(k, ln) for k in kinds), ln
    for decl in ("void rollout_linearized_device(", "void rollout_linearized_kernel(", "void rollout_linearized_reserve(", "void rollout_kernel(", "void close_grid("):
        assert sum(decl in ln for ln in lines[:start] + lines[end + 1:]) == 1, decl


def test_prismatic_tree_adjoint():
    robot = _rnd_prismatic()
    lib = emu_library(robot)
    x0, u = inputs(robot.n, 3, 6, 12)
    g = cotangent(robot.n, 3, 6, 12)
    traj = lib.rollout_host(x0, u, DT)
    gx0, gu = lib.rollout_adjoint_host(traj, u, DT, gx=g)
    check("random prismatic tree", robot, traj, u, gx0, gu, ATOL32, gx=g)
    lib.close()


# ---------------------------------------------------------------------------------------------------- 10. the emitted host wrappers
def test_generated_host_wrappers_under_emulation(tmp_path):
    """tests/cpp/host_api_rollout_adjoint_demo.hip compiled against the emulation: the emitted host wrappers give what the C ABI gives"""
    from gridcodegenerator_amd.runtime import generate_header

    here = os.path.dirname(os.path.abspath(__file__))
    name, n, Nd, S = "iiwa14", 7, 11, 6
    generate_header(RobotModel.from_fixture(name), str(tmp_path / "gen"))
    exe = str(tmp_path / "demo")
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-pthread", "-I" + os.path.join(here, "emu"), "-I" + str(tmp_path / "gen"), "-x", "c++",
                           os.path.join(here, "cpp", "host_api_rollout_adjoint_demo.hip"), "-o", exe])
    x0, u = inputs(n, Nd, S, 14)
    g = cotangent(n, Nd, S, 14)
    (tmp_path / "x0.bin").write_bytes(np.hstack([x0, np.zeros((Nd, n), np.float32)]).astype(np.float64).tobytes())
    (tmp_path / "u.bin").write_bytes(u.astype(np.float64).tobytes())
    (tmp_path / "gx.bin").write_bytes(g.astype(np.float64).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "x0.bin"), str(tmp_path / "u.bin"), str(tmp_path / "gx.bin"), str(Nd), str(S), repr(DT), str(tmp_path / "f32.bin"),
                                   str(tmp_path / "f64.bin")], text=True, timeout=600)
    assert out.count("Single Call ROLLOUT_ADJ") == 2
    assert out.count("max|delta|") == 4
    for line in out.splitlines():
        if "max|delta|" in line:
            assert float(line.split("=")[-1]) == 0.0, line
    lib = emu_library(name)
    for fname, dtype, roll, adj in (("f32.bin", np.float32, lib.rollout_host, lib.rollout_adjoint_host), ("f64.bin", np.float64, lib.rollout_host_f64, lib.rollout_adjoint_host_f64)):
        got = np.frombuffer((tmp_path / fname).read_bytes(), dtype=np.float64)
        traj = roll(x0.astype(dtype), u.astype(dtype), DT)
        ref = np.concatenate([a.astype(np.float64).reshape(-1) for a in (traj,) + adj(traj, u.astype(dtype), DT, gx=g.astype(dtype))])
        assert got.shape == ref.shape and np.abs(got - ref).max() == 0.0, fname
    lib.close()


# ---------------------------------------------------------------------------------------------------- 11. rollout_torch on CPU tensors
@pytest.mark.parametrize("name", ["iiwa14", "hyq"])
@pytest.mark.parametrize("shared", [False, True])
def test_rollout_torch_gradcheck(name, shared, libs):
    import torch

    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, 2, 3, 19, np.float64)
    tx = torch.from_numpy(x0).requires_grad_(True)
    tu = torch.from_numpy(np.ascontiguousarray(u[:, 0]) if shared else u).requires_grad_(True)
    fn = lambda a, b: lib.rollout_torch(a, b, DT)
    traj = fn(tx, tu)
    assert traj.shape == (4, 2, 2 * n) and traj.dtype == torch.float64 and traj.requires_grad
    assert np.array_equal(traj.detach().numpy(), lib.rollout_host_f64(x0, tu.detach().numpy(), DT))
    # forward is rollout (ABA), backward linearises the forward-dynamics-gradient formulation of the same map: they agree to rounding, and gradcheck's central
    # differences (eps 1e-6) on a map whose Jacobian has entries of order 1 are good to about 1e-8.  fast_mode: random projections of the Jacobian instead of one
    # emulated launch per input and per output element (minutes per case under the thread-per-lane emulation)
    assert torch.autograd.gradcheck(fn, (tx, tu), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0, fast_mode=True)


def test_rollout_torch_float32_backward_against_the_reference(libs):
    import torch

    name = "hyq"
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 21)
    g = cotangent(n, N, T, 21)
    tx, tu = torch.from_numpy(x0).requires_grad_(True), torch.from_numpy(u).requires_grad_(True)
    traj = lib.rollout_torch(tx, tu, DT)
    assert traj.dtype == torch.float32 and np.array_equal(traj.detach().numpy(), lib.rollout_host(x0, u, DT))
    (traj * torch.from_numpy(g)).sum().backward()
    check(name + " rollout_torch fp32", name, traj.detach().numpy(), u, tx.grad.numpy(), tu.grad.numpy(), ATOL32, gx=g)
    # shared control: the gradient of the one sequence is the sum of the per-solve gradients
    ts = torch.from_numpy(np.ascontiguousarray(u[:, 0])).requires_grad_(True)
    tr = lib.rollout_torch(torch.from_numpy(x0), ts, DT)
    (tr * torch.from_numpy(g)).sum().backward()
    _, ru = oracle_adjoint(name, tr.detach().numpy(), ts.detach().numpy(), DT, gx=g)
    rs = ru.sum(axis=1)
    assert ts.grad.shape == (T, n) and np.abs(ts.grad.numpy() - rs).max() <= ATOL32 * np.abs(rs).max() * N  # (a sum of N records, each inside the bar)


def test_rollout_torch_computes_only_what_is_asked_and_refuses_double_backward(libs, monkeypatch):
    import torch

    lib = libs("iiwa14")
    n = lib.n
    x0, u = inputs(n, 3, 4, 22, np.float64)
    seen = []
    real = lib.rollout_adjoint_host_f64
    monkeypatch.setattr(lib, "rollout_adjoint_host_f64", lambda *a, **kw: (seen.append(tuple(kw["want"])), real(*a, **kw))[1])
    tx, tu = torch.from_numpy(x0).requires_grad_(True), torch.from_numpy(u)
    lib.rollout_torch(tx, tu, DT).sum().backward()
    assert seen == [("grad_x0",)] and tx.grad is not None and tu.grad is None
    seen.clear()
    tx, tu = torch.from_numpy(x0), torch.from_numpy(u).requires_grad_(True)
    lib.rollout_torch(tx, tu, DT).sum().backward()
    assert seen == [("grad_u",)] and tu.grad.shape == u.shape
    assert not lib.rollout_torch(torch.from_numpy(x0), torch.from_numpy(u), DT).requires_grad
    # T = 0
    tx = torch.from_numpy(x0).requires_grad_(True)
    t0 = lib.rollout_torch(tx, torch.zeros((0, 3, n), dtype=torch.float64, requires_grad=True), DT)
    assert t0.shape == (1, 3, 2 * n)
    t0.sum().backward()
    assert torch.equal(tx.grad, torch.ones_like(tx))
    # double backward raises
    tx, tu = torch.from_numpy(x0).requires_grad_(True), torch.from_numpy(u).requires_grad_(True)
    (gx,) = torch.autograd.grad(lib.rollout_torch(tx, tu, DT).sum(), tx, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiable once"):
        gx.sum().backward()
    with pytest.raises((TypeError, ValueError)):
        lib.rollout_torch(torch.from_numpy(x0), torch.from_numpy(u).float(), DT)
    with pytest.raises(ValueError):
        lib.rollout_torch(torch.from_numpy(x0[:, :n]), torch.from_numpy(u), DT)
