"""Linearised rollout on the GPU (run with -m gpu on an MI355X), through the C ABI (include/grid_capi.h) and the ctypes binding.

Reference: tests/rollout_linearized_reference.py - the fp64 oracle stepped in NumPy fp64 for the states; Oracle.fd_grad(q, qd, u, full=True) for the Jacobians,
evaluated at the state the kernel returned (traj[t, k] cast to fp64) with u[t, k]: a Jacobian check measures the Jacobian, not trajectory drift.
Bars: states per solve max|d| / max(1, max|ref|) <= 1e-4 (fp32), 1e-9 (fp64); Jacobians per record max|got - ref| <= 1e-4 max|ref| (fp32), 1e-9 (fp64), fx and
fu each on their own; every solve and every step compared, NaN / inf on either side fails.  Inputs q0, qd0 ~ U(-1, 1), u ~ U(-5, 5), dt = 1e-3, T = 64.

Room under the bar at the test's own N = 1000 and seed 31, from the reference alone: Oracle(robot, np.float32) against the fp64 oracle on all 64 000 records of the
fp64 oracle trajectories, worst per-record fx / fu: iiwa14 2.3e-6 / 1.3e-7, hyq 9.8e-7 / 2.1e-7, atlas 2.5e-6 / 2.2e-7, mixed5 1.5e-6 / 3.2e-7, arm6 4.2e-6 / 1.0e-7,
chain12 3.8e-6 / 1.2e-7, chain8 2.9e-6 / 1.8e-7, tree12 7.1e-6 / 2.1e-7 - at least 14x inside 1e-4; all states finite (max|qd| reaches 448 on arm6, 102 on tree12,
88 on atlas by step 64).

Discrete Jacobians (no oracle involved): tolerance = 10x the oracle-only figure on the same states, see tests/test_rollout_linearized.py.
On the GPU fx[t] is compared with forward_dynamics_gradient_device at (traj[t], u[t]) and fu[t] with direct_minv_device within the bar: the compiler is free to
schedule and contract the inlined device functions differently inside the step loop than inside the stand-alone kernels.  (Measured on an MI355X: both came out
bit-identical on iiwa14, hyq, atlas and mixed5, all 64 000 records each; bit-identity is asserted under the emulation only.)

Measured on an MI355X (fp32, worst per record over 64 000 records, states / fx / fu): iiwa14 3.7e-7 / 1.05e-5 / 1.6e-7, hyq 5.5e-7 / 3.0e-6 / 4.5e-7, atlas 6.7e-7 / 4.8e-6 /
8.3e-7, mixed5 7.8e-7 / 9.5e-7 / 2.5e-7, arm6 4.2e-7 / 4.9e-6 / 1.7e-7, chain12 7.6e-7 / 6.1e-6 / 3.2e-7, chain8 6.5e-7 / 3.9e-6 / 2.7e-7, tree12 5.4e-7 / 7.6e-6 / 3.0e-7; fp64
states <= 1.5e-15, fx <= 2.9e-14, fu <= 2.0e-15.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gridcodegenerator_amd import RobotModel
from gridcodegenerator_amd.runtime import HIPCC_FLAGS, GridLibrary, build_library, discrete_jacobians, generate_header
from rollout_linearized_reference import JTOL32, JTOL64, oracle_jacobians, per_record_err
from rollout_reference import FIXTURES, TOL32, TOL64, inputs, oracle_rollout, per_solve_err

pytestmark = pytest.mark.gpu
T, DT = 64, 1e-3
MAX_N = 16384
FD_TOL = {"iiwa14": (8.6e-9, 4.1e-9), "hyq": (9.4e-10, 5.5e-10), "chain8": (1.5e-9, 8.5e-10), "tree12": (1.2e-7, 4.5e-8), "mixed5": (None, 5.4e-10)}  # (tests/test_rollout_linearized.py)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def libs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = GridLibrary(build_library(name), device=0, max_timesteps=MAX_N)  # raises when the HIP .so is missing
        return cache[name]

    yield get
    for lib in cache.values():
        lib.close()


def report(tag, err):
    print("[rollout_linearized parity] %s: worst %.3g, p99.9 %.3g over %d" % (tag, err.max(), np.quantile(err, 0.999), err.size))


def check_jacobians(tag, name, traj, u, fx, fu, tol):
    rfx, rfu = oracle_jacobians(name, traj, u)
    efx, efu = per_record_err(fx, rfx), per_record_err(fu, rfu)
    report(tag + " fx", efx)
    report(tag + " fu", efu)
    assert efx.max() <= tol and efu.max() <= tol, (tag, efx.max(), efu.max())


@pytest.mark.parametrize("name", FIXTURES)
def test_rollout_linearized_matches_the_oracle(name, torch_cuda, libs):
    """N = 1000 (a partial last block), every solve, every step, every record; fp32 and the fp64 twin"""
    lib = libs(name)
    n, N = lib.n, 1000
    x0, u = inputs(n, N, T, 31)
    ref = oracle_rollout(name, x0, u, DT)
    traj, fx, fu = lib.rollout_linearized_host(x0, u, DT)
    assert np.array_equal(traj[0], x0)
    err = per_solve_err(traj, ref)
    report(name + " fp32 states", err)
    assert err.max() <= TOL32
    check_jacobians(name + " fp32", name, traj, u, fx, fu, JTOL32)
    F = fu.reshape(T, N, n, n)
    assert np.array_equal(F, F.swapaxes(-1, -2))
    x64, u64 = x0.astype(np.float64), u.astype(np.float64)
    t64, fx64, fu64 = lib.rollout_linearized_host_f64(x64, u64, DT)
    assert np.array_equal(t64[0], x64)
    err64 = per_solve_err(t64, ref)
    report(name + " fp64 states", err64)
    assert err64.max() <= TOL64
    check_jacobians(name + " fp64", name, t64, u64, fx64, fu64, JTOL64)
    F = fu64.reshape(T, N, n, n)
    assert np.array_equal(F, F.swapaxes(-1, -2))


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "atlas", "mixed5"])
def test_agrees_with_the_stepwise_entry_points(name, torch_cuda, libs):
    """What a user does today, same inputs: forward_dynamics_gradient_device and direct_minv_device at (traj[t], u[t]), rollout for the states"""
    torch = torch_cuda
    lib = libs(name)
    n, N = lib.n, 1000
    x0, u = inputs(n, N, T, 24)
    st = torch.cuda.current_stream().cuda_stream
    d_x0, d_u = torch.from_numpy(x0).cuda(), torch.from_numpy(u).cuda()
    d_traj = torch.full((T + 1, N, 2 * n), float("nan"), dtype=torch.float32, device="cuda")
    d_fx = torch.full((T, N, 2 * n * n), float("nan"), dtype=torch.float32, device="cuda")
    d_fu = torch.full((T, N, n * n), float("nan"), dtype=torch.float32, device="cuda")
    d_roll = torch.zeros_like(d_traj)
    lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_traj=d_traj, d_fx=d_fx, d_fu=d_fu, stream=st)
    lib.rollout_device(d_x0, d_u, N, T, DT, d_traj=d_roll, stream=st)
    d_x = torch.zeros((N, 3 * n), dtype=torch.float32, device="cuda")
    d_g = torch.zeros((T, N, 2 * n * n), dtype=torch.float32, device="cuda")
    d_m = torch.zeros((T, N, n * n), dtype=torch.float32, device="cuda")
    for t in range(T):
        d_x[:, :2 * n] = d_traj[t]
        d_x[:, 2 * n:] = d_u[t]
        lib.forward_dynamics_gradient_device(d_x, N, d_g[t], stream=st)
        lib.direct_minv_device(d_x, N, d_m[t], stream=st)
    torch.cuda.synchronize()
    err = per_solve_err(d_traj.cpu().numpy(), d_roll.cpu().numpy().astype(np.float64))
    report(name + " states vs rollout", err)
    assert err.max() <= TOL32
    e = per_record_err(d_fx.cpu().numpy(), d_g.cpu().numpy())
    report(name + " fx vs forward_dynamics_gradient_device", e)
    assert e.max() <= JTOL32
    iu = np.triu_indices(n)
    got, ref = d_fu.cpu().numpy().reshape(T, N, n, n)[..., iu[1], iu[0]], d_m.cpu().numpy().reshape(T, N, n, n)[..., iu[1], iu[0]]
    e = per_record_err(got, ref)
    report(name + " fu vs direct_minv_device (upper triangle)", e)
    assert e.max() <= JTOL32


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "chain8", "tree12", "mixed5"])
def test_discrete_jacobians_against_central_differences_of_the_own_step(name, torch_cuda, libs):
    lib = libs(name)
    n = lib.n
    K, h = 6, 1e-6
    x0, u = inputs(n, K, 1, 41, np.float64)
    _, fx, fu = lib.rollout_linearized_host_f64(x0, u, DT)
    A, B = discrete_jacobians(fx[0], fu[0], DT)
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
    eA, eB = np.abs(fd[:, :2 * n].swapaxes(1, 2) - A).max(), np.abs(fd[:, 2 * n:].swapaxes(1, 2) - B).max()
    print("[rollout_linearized layout] %s: max|A - fd| %.3g, max|B - fd| %.3g" % (name, eA, eB))
    tolA, tolB = FD_TOL[name]
    assert eB <= tolB
    if tolA is not None:  # (non-root prismatic joints: fx follows the oracle, whose d/dq is not the derivative there)
        assert eA <= tolA


@pytest.mark.parametrize("name,N", [("iiwa14", 16384), ("hyq", 4096)])
def test_torch_tensors_on_a_side_stream_modes_and_composition(name, N, torch_cuda, libs):
    """The configured batches: every output mode bit-identical to the all-outputs call, shared control, (N, 3n) rows, composition 24 + 40, and every record of a
    256-solve random subset against the oracle - outputs NaN-prefilled"""
    torch = torch_cuda
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 23)
    side = torch.cuda.Stream()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    same = lambda a, b: torch.equal(a, b) and not bool(torch.isnan(a).any())
    with torch.cuda.stream(side):
        s = side.cuda_stream
        d_x0 = torch.from_numpy(np.hstack([x0, np.full((N, n), 1e9, np.float32)])).cuda()  # (N, 3n) rows as they are; the third block is not read
        d_u = torch.from_numpy(u).cuda()
        d_traj, d_xT, d_fx, d_fu = nan(T + 1, N, 2 * n), nan(N, 2 * n), nan(T, N, 2 * n * n), nan(T, N, n * n)
        lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_traj=d_traj, d_xT=d_xT, d_fx=d_fx, d_fu=d_fu, stride_x0=3 * n, stream=s)
        side.synchronize()
        assert torch.equal(d_traj[0], d_x0[:, :2 * n]) and same(d_traj[T], d_xT)
        # one output at a time, through ONE scratch buffer per kind
        o = nan(T, N, 2 * n * n)
        lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_fx=o, stride_x0=3 * n, stream=s)
        side.synchronize()
        assert same(o, d_fx)
        # composition: 24 steps, then 40 more from that state - fx rows bit for bit
        o.fill_(float("nan"))
        d_mid = nan(N, 2 * n)
        lib.rollout_linearized_device(d_x0, d_u, N, 24, DT, d_xT=d_mid, d_fx=o[:24], stride_x0=3 * n, stream=s)
        lib.rollout_linearized_device(d_mid, d_u[24:], N, T - 24, DT, d_fx=o[24:], stream=s)
        side.synchronize()
        assert same(d_mid, d_traj[24]) and same(o, d_fx)
        del o
        o = nan(T, N, n * n)
        lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_fu=o, stride_x0=3 * n, stream=s)
        side.synchronize()
        assert same(o, d_fu)
        o.fill_(float("nan"))
        d_end = nan(N, 2 * n)
        lib.rollout_linearized_device(d_x0, d_u, N, 24, DT, d_fu=o[:24], stride_x0=3 * n, stream=s)
        lib.rollout_linearized_device(d_mid, d_u[24:], N, T - 24, DT, d_xT=d_end, d_fu=o[24:], stream=s)
        side.synchronize()
        assert same(o, d_fu) and same(d_end, d_xT)
        del o
        o, o2 = nan(T + 1, N, 2 * n), nan(N, 2 * n)
        lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_traj=o, stride_x0=3 * n, stream=s)
        lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_xT=o2, stride_x0=3 * n, stream=s)
        side.synchronize()
        assert same(o, d_traj) and same(o2, d_xT)
        # one control sequence for all solves == the tiled one
        d_shared = d_u[:, 0].contiguous()
        d_tiled = d_shared[:, None, :].expand(T, N, n).contiguous()
        a_x, a_fu, b_x, b_fu = nan(N, 2 * n), nan(T, N, n * n), nan(N, 2 * n), nan(T, N, n * n)
        lib.rollout_linearized_device(d_x0, d_shared, N, T, DT, d_xT=a_x, d_fu=a_fu, stride_x0=3 * n, u_shared=True, stream=s)
        lib.rollout_linearized_device(d_x0, d_tiled, N, T, DT, d_xT=b_x, d_fu=b_fu, stride_x0=3 * n, stream=s)
        side.synchronize()
        assert same(a_x, b_x) and same(a_fu, b_fu)
    # every record of a random 256-solve subset against the oracle
    pick = np.sort(np.random.default_rng(29).choice(N, 256, replace=False))
    d_pick = torch.from_numpy(pick).cuda()
    traj, fx, fu = (a[:, d_pick].cpu().numpy() for a in (d_traj, d_fx, d_fu))
    err = per_solve_err(traj, oracle_rollout(name, x0[pick], u[:, pick], DT))
    report("%s @%d states (256 solves)" % (name, N), err)
    assert err.max() <= TOL32
    check_jacobians("%s @%d (256 solves)" % (name, N), name, traj, u[:, pick], fx, fu, JTOL32)
    F = d_fu.reshape(T, N, n, n)
    assert torch.equal(F, F.transpose(-1, -2))


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "atlas"])
def test_a_diverging_solve_does_not_poison_its_neighbours(name, torch_cuda, libs):
    lib = libs(name)
    N = 1000
    x0, u = inputs(lib.n, N, T, 13)
    clean = lib.rollout_linearized_host(x0, u, DT)
    u_bad = u.copy()
    u_bad[:, 2] = 1e30
    bad = lib.rollout_linearized_host(x0, u_bad, DT)
    assert not np.isfinite(bad[0][T, 2]).all()  # plain floating point: inf / NaN, nothing faults
    others = np.arange(N) != 2
    for a, b in zip(bad, clean):
        assert np.array_equal(a[:, others], b[:, others])


@pytest.mark.parametrize("name", ["iiwa14", "tree12"])
def test_generated_host_api_demo(name, tmp_path, torch_cuda, libs):
    """A hipcc-compiled downstream program calling the emitted rollout_linearized<T> host wrappers gets what the C ABI gives (max|delta| = 0), fp32 and fp64"""
    lib = libs(name)
    n = lib.n
    Nd, S = 500, 16
    x0, u = inputs(n, Nd, S, 25)
    gen_dir = tmp_path / "gen"
    generate_header(RobotModel.from_fixture(name), str(gen_dir))
    exe = str(tmp_path / "host_api_rollout_linearized_demo")
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "host_api_rollout_linearized_demo.hip")
    subprocess.check_call([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + flags + ["-I" + str(gen_dir), src, "-o", exe])
    (tmp_path / "x0.bin").write_bytes(np.hstack([x0, np.zeros((Nd, n), np.float32)]).astype(np.float64).tobytes())
    (tmp_path / "u.bin").write_bytes(u.astype(np.float64).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "x0.bin"), str(tmp_path / "u.bin"), str(Nd), str(S), repr(DT), str(tmp_path / "f32.bin"), str(tmp_path / "f64.bin")],
                                  text=True, timeout=300)
    assert out.count("Single Call ROLLOUT_LIN") == 2 and out.count("max|delta|") == 4
    for line in out.splitlines():
        if "max|delta|" in line:
            assert float(line.split("=")[-1]) == 0.0, line
    for fname, dtype, fn in (("f32.bin", np.float32, lib.rollout_linearized_host), ("f64.bin", np.float64, lib.rollout_linearized_host_f64)):
        got = np.frombuffer((tmp_path / fname).read_bytes(), dtype=np.float64)
        ref = np.concatenate([a.astype(np.float64).reshape(-1) for a in fn(x0.astype(dtype), u.astype(dtype), DT)])
        assert got.shape == ref.shape and np.abs(got - ref).max() == 0.0, fname
