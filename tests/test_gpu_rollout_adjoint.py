"""Rollout adjoint on the GPU (run with -m gpu on an MI355X), through the C ABI (include/grid_capi.h), the ctypes binding and rollout_torch.

Reference: tests/rollout_adjoint_reference.py - A_t, B_t from rollout_linearized_reference.block_jacobians of the fp64 oracle's Jacobians at the traj and u handed to
the kernel (traj is an input of the adjoint: reference and kernel see the same states), then lam_t = g_t + A_t^T lam_{t+1}, grad_u_t = B_t^T lam_{t+1} in fp64.
Error per solve: max|d| / max|ref| over the solve's grad_x0 record and over all (t, j) of its grad_u, each on its own; NaN / inf on either side fails.
Bars: 1e-4 (fp32), 1e-9 (fp64).  Inputs q0, qd0 ~ U(-1, 1), u ~ U(-5, 5), g ~ U(-1, 1) at every step, dt = 1e-3, T = 64, no solve skipped.

Room under the bar from the reference alone (Oracle(robot, np.float32) against the fp64 oracle on such inputs, T = 64, worst solve, grad_x0 / grad_u): iiwa14 7.7e-7 /
1.9e-7, hyq 3.0e-7 / 2.8e-7, atlas 7.2e-7 / 2.0e-7, mixed5 3.2e-7 / 3.1e-7, arm6 6.6e-7 / 2.2e-7, chain12 4.2e-7 / 3.0e-7, chain8 5.6e-7 / 4.4e-7, tree12 1.1e-6 / 2.1e-7:
at least 90x inside 1e-4.

The parent's route (rollout_linearized_device writing fx + fu, discrete_jacobians, a torch reverse loop) on the same traj is held to the same bar against the
kernel: both are fp32 evaluations of one recurrence with differently ordered sums.

Measured on an MI355X (fp32, worst solve of 1 000, grad_x0 / grad_u): iiwa14 9.0e-6 / 5.5e-7, hyq 7.9e-7 / 9.5e-7, atlas 6.4e-6 / 9.9e-7, mixed5 8.7e-7 / 2.0e-6, arm6 2.7e-6 / 7.4e-7,
chain12 3.5e-6 / 1.2e-6, chain8 1.6e-6 / 1.0e-6, tree12 4.8e-6 / 6.8e-7; fp64 grad_x0 <= 2.2e-14, grad_u <= 3.1e-15; against the parent's route <= 2.3e-6 / 1.8e-6.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from gridcodegenerator_amd import RobotModel
from gridcodegenerator_amd.runtime import HIPCC_FLAGS, GridLibrary, build_library, discrete_jacobians, generate_header
from rollout_adjoint_reference import ATOL32, ATOL64, cotangent, oracle_adjoint, per_solve_err
from rollout_reference import FIXTURES, inputs

pytestmark = pytest.mark.gpu
T, DT = 64, 1e-3
MAX_N = 16384
PARITY_LOG = os.environ.get("GRID_ADJOINT_PARITY_LOG")  # optional: a .jsonl the parity test appends its figures to (profiles/r08_rollout_adjoint_parity.jsonl was written so)


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
    print("[rollout_adjoint parity] %s: worst %.3g, p99.9 %.3g over %d" % (tag, err.max(), np.quantile(err, 0.999), err.size))
    return {"worst": float(err.max()), "p999": float(np.quantile(err, 0.999)), "solves": int(err.size)}


def check(tag, name, traj, u, got_x0, got_u, tol, **cot):
    rx0, ru = oracle_adjoint(name, traj, u, DT, **cot)
    ex, eu = per_solve_err(got_x0, rx0), per_solve_err(got_u, ru)
    rec = {"grad_x0": report(tag + " grad_x0", ex), "grad_u": report(tag + " grad_u", eu)}
    assert ex.max() <= tol and eu.max() <= tol, (tag, ex.max(), eu.max())
    return rec


@pytest.mark.parametrize("name", FIXTURES)
def test_rollout_adjoint_matches_the_reference(name, torch_cuda, libs):
    """N = 1000 (a partial last block), every solve; fp32 and the fp64 twin"""
    lib = libs(name)
    n, N = lib.n, 1000
    x0, u = inputs(n, N, T, 31)
    g = cotangent(n, N, T, 31)
    traj = lib.rollout_host(x0, u, DT)
    gx0, gu = lib.rollout_adjoint_host(traj, u, DT, gx=g)
    r32 = check(name + " fp32", name, traj, u, gx0, gu, ATOL32, gx=g)
    x64, u64, g64 = x0.astype(np.float64), u.astype(np.float64), g.astype(np.float64)
    t64 = lib.rollout_host_f64(x64, u64, DT)
    a0, au = lib.rollout_adjoint_host_f64(t64, u64, DT, gx=g64)
    r64 = check(name + " fp64", name, t64, u64, a0, au, ATOL64, gx=g64)
    if PARITY_LOG:
        with open(PARITY_LOG, "a") as f:
            f.write(json.dumps({"robot": name, "solves": N, "steps": T, "dt": DT, "fp32": r32, "fp64": r64}) + "\n")


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "atlas", "mixed5"])
def test_agrees_with_the_route_of_the_parent(name, torch_cuda, libs):
    """What a user did before: rollout_linearized_device writing fx + fu, discrete_jacobians, the recurrence as a torch loop - same traj, same u, same g"""
    torch = torch_cuda
    lib = libs(name)
    n, N = lib.n, 1000
    x0, u = inputs(n, N, T, 24)
    g = cotangent(n, N, T, 24)
    st = torch.cuda.current_stream().cuda_stream
    d_x0, d_u, d_g = torch.from_numpy(x0).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(g).cuda()
    d_traj = torch.empty((T + 1, N, 2 * n), dtype=torch.float32, device="cuda")
    d_fx = torch.empty((T, N, 2 * n * n), dtype=torch.float32, device="cuda")
    d_fu = torch.empty((T, N, n * n), dtype=torch.float32, device="cuda")
    lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_traj=d_traj, d_fx=d_fx, d_fu=d_fu, stream=st)
    A, B = discrete_jacobians(d_fx, d_fu, DT)
    lam = d_g[T].clone()
    ref_u = torch.empty((T, N, n), dtype=torch.float32, device="cuda")
    for t in range(T - 1, -1, -1):
        ref_u[t] = torch.einsum("kij,ki->kj", B[t], lam)
        lam = d_g[t] + torch.einsum("kij,ki->kj", A[t], lam)
    d_gx0 = torch.full((N, 2 * n), float("nan"), dtype=torch.float32, device="cuda")
    d_gu = torch.full((T, N, n), float("nan"), dtype=torch.float32, device="cuda")
    lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_g, d_grad_x0=d_gx0, d_grad_u=d_gu, stream=st)
    torch.cuda.synchronize()
    ex = per_solve_err(d_gx0.cpu().numpy(), lam.cpu().numpy())
    eu = per_solve_err(d_gu.cpu().numpy(), ref_u.cpu().numpy())
    report(name + " grad_x0 vs rollout_linearized + torch loop", ex)
    report(name + " grad_u vs rollout_linearized + torch loop", eu)
    assert ex.max() <= ATOL32 and eu.max() <= ATOL32


@pytest.mark.parametrize("name,N", [("iiwa14", 16384), ("hyq", 4096)])
def test_torch_tensors_on_a_side_stream_modes_positions_determinism(name, N, torch_cuda, libs):
    """The configured batches, outputs NaN-prefilled: every mode bit-identical to the all-outputs call, shared control, a solve gives the same record wherever it
    sits in the batch, two runs are bit-identical, and every record of a 256-solve random subset against the reference"""
    torch = torch_cuda
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 23)
    g = cotangent(n, N, T, 23)
    side = torch.cuda.Stream()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    same = lambda a, b: torch.equal(a, b) and not bool(torch.isnan(a).any())
    with torch.cuda.stream(side):
        s = side.cuda_stream
        d_x0, d_u, d_g = torch.from_numpy(x0).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(g).cuda()
        d_traj = nan(T + 1, N, 2 * n)
        lib.rollout_device(d_x0, d_u, N, T, DT, d_traj=d_traj, stream=s)
        d_gx0, d_gu = nan(N, 2 * n), nan(T, N, n)
        lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_g, d_grad_x0=d_gx0, d_grad_u=d_gu, stream=s)
        side.synchronize()
        assert not bool(torch.isnan(d_gx0).any()) and not bool(torch.isnan(d_gu).any())
        # determinism: a second run into fresh buffers
        o0, ou = nan(N, 2 * n), nan(T, N, n)
        lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_g, d_grad_x0=o0, d_grad_u=ou, stream=s)
        side.synchronize()
        assert same(o0, d_gx0) and same(ou, d_gu)
        # one output at a time
        o0.fill_(float("nan"))
        ou.fill_(float("nan"))
        lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_g, d_grad_x0=o0, stream=s)
        lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_g, d_grad_u=ou, stream=s)
        side.synchronize()
        assert same(o0, d_gx0) and same(ou, d_gu)
        # the last row of gx moved to gxT
        d_head, d_gT = d_g.clone(), d_g[T].clone()
        d_head[T] = 0
        o0.fill_(float("nan"))
        ou.fill_(float("nan"))
        lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_head, d_gxT=d_gT, d_grad_x0=o0, d_grad_u=ou, stream=s)
        side.synchronize()
        assert same(o0, d_gx0) and same(ou, d_gu)
        # gxT alone == gx that is zero before the last row
        d_tail = torch.zeros_like(d_g)
        d_tail[T] = d_g[T]
        a0, au, b0, bu = nan(N, 2 * n), nan(T, N, n), nan(N, 2 * n), nan(T, N, n)
        lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gxT=d_gT, d_grad_x0=a0, d_grad_u=au, stream=s)
        lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_tail, d_grad_x0=b0, d_grad_u=bu, stream=s)
        side.synchronize()
        assert same(a0, b0) and same(au, bu)
        # composition: the last 40 steps, then the first 24 with gxT = lam_24 (g at 24 counted once)
        lam, o0 = nan(N, 2 * n), nan(N, 2 * n)
        ou.fill_(float("nan"))
        lib.rollout_adjoint_device(d_traj[24:], d_u[24:], N, T - 24, DT, d_gx=d_g[24:], d_grad_x0=lam, d_grad_u=ou[24:], stream=s)
        d_first = d_g[:25].clone()
        d_first[24] = 0
        lib.rollout_adjoint_device(d_traj[:25], d_u[:24], N, 24, DT, d_gx=d_first, d_gxT=lam, d_grad_x0=o0, d_grad_u=ou[:24], stream=s)
        side.synchronize()
        assert same(o0, d_gx0) and same(ou, d_gu)
        # batch-position independence: the batch reversed gives the reversed records
        r_traj, r_u, r_g = d_traj.flip(1).contiguous(), d_u.flip(1).contiguous(), d_g.flip(1).contiguous()
        o0.fill_(float("nan"))
        ou.fill_(float("nan"))
        lib.rollout_adjoint_device(r_traj, r_u, N, T, DT, d_gx=r_g, d_grad_x0=o0, d_grad_u=ou, stream=s)
        side.synchronize()
        assert same(o0.flip(0), d_gx0) and same(ou.flip(1), d_gu)
        del r_traj, r_u, r_g
        # one control sequence for all solves == the tiled one (grad_u per solve in both)
        d_shared = d_u[:, 0].contiguous()
        d_tiled = d_shared[:, None, :].expand(T, N, n).contiguous()
        lib.rollout_device(d_x0, d_shared, N, T, DT, d_traj=(s_traj := nan(T + 1, N, 2 * n)), u_shared=True, stream=s)
        lib.rollout_adjoint_device(s_traj, d_shared, N, T, DT, d_gx=d_g, d_grad_x0=a0, d_grad_u=au, u_shared=True, stream=s)
        lib.rollout_adjoint_device(s_traj, d_tiled, N, T, DT, d_gx=d_g, d_grad_x0=b0, d_grad_u=bu, stream=s)
        side.synchronize()
        assert same(a0, b0) and same(au, bu)
    pick = np.sort(np.random.default_rng(29).choice(N, 256, replace=False))
    d_pick = torch.from_numpy(pick).cuda()
    check("%s @%d (256 solves)" % (name, N), name, d_traj[:, d_pick].cpu().numpy(), u[:, pick], d_gx0[d_pick].cpu().numpy(), d_gu[:, d_pick].cpu().numpy(), ATOL32, gx=g[:, pick])


@pytest.mark.parametrize("name,N", [("iiwa14", 16384), ("hyq", 4096)])
def test_rollout_torch_on_cuda_tensors(name, N, torch_cuda, libs):
    """rollout_torch on CUDA tensors against the same call on CPU tensors (host entry points): same kernels, same inputs - bit-identical; shared u summed over N"""
    torch = torch_cuda
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 27)
    g = cotangent(n, N, T, 27)
    res = {}
    for dev in ("cpu", "cuda"):
        tx, tu = torch.from_numpy(x0).to(dev).requires_grad_(True), torch.from_numpy(u).to(dev).requires_grad_(True)
        traj = lib.rollout_torch(tx, tu, DT)
        (traj * torch.from_numpy(g).to(dev)).sum().backward()
        res[dev] = (traj.detach().cpu(), tx.grad.cpu(), tu.grad.cpu())
    assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(res["cpu"], res["cuda"]))
    pick = np.sort(np.random.default_rng(30).choice(N, 128, replace=False))
    check("%s rollout_torch @%d (128 solves)" % (name, N), name, res["cuda"][0].numpy()[:, pick], u[:, pick], res["cuda"][1].numpy()[pick], res["cuda"][2].numpy()[:, pick],
          ATOL32, gx=g[:, pick])
    # fp64 and a shared control on the device: the gradient of the one sequence is the sum over the solves
    K = 512
    x64, us64, g64 = x0[:K].astype(np.float64), u[:, 0].astype(np.float64), g[:, :K].astype(np.float64)
    tx, ts = torch.from_numpy(x64).cuda().requires_grad_(True), torch.from_numpy(us64).cuda().requires_grad_(True)
    traj = lib.rollout_torch(tx, ts, DT)
    assert traj.dtype == torch.float64 and traj.is_cuda
    (traj * torch.from_numpy(g64).cuda()).sum().backward()
    r0, ru = oracle_adjoint(name, traj.detach().cpu().numpy(), us64, DT, gx=g64)
    assert per_solve_err(tx.grad.cpu().numpy(), r0).max() <= ATOL64
    rs = ru.sum(axis=1)
    assert ts.grad.shape == (T, n) and np.abs(ts.grad.cpu().numpy() - rs).max() <= ATOL64 * np.abs(ru).max() * K  # (a sum of K records, each inside the bar)
    # only what is asked for; double backward raises
    tx, tu = torch.from_numpy(x0[:K]).cuda().requires_grad_(True), torch.from_numpy(u[:, :K]).cuda()
    lib.rollout_torch(tx, tu, DT).sum().backward()
    assert tx.grad is not None and tu.grad is None
    tx = torch.from_numpy(x0[:K]).cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(lib.rollout_torch(tx, tu, DT).sum(), tx, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiable once"):
        gx.sum().backward()


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "atlas"])
def test_diverging_solves_do_not_poison_their_neighbours(name, torch_cuda, libs):
    lib = libs(name)
    n, N = lib.n, 1000
    x0, u = inputs(n, N, T, 13)
    g = cotangent(n, N, T, 13)
    traj = lib.rollout_host(x0, u, DT)
    clean = lib.rollout_adjoint_host(traj, u, DT, gx=g)
    tb, ub, gb = traj.copy(), u.copy(), g.copy()
    tb[20, 2] = np.nan      # a NaN state in solve 2
    gb[T, 501, 0] = np.inf  # an infinite cotangent in solve 501
    ub[:, 999] = 3e38       # overflowing controls in solve 999
    bad = lib.rollout_adjoint_host(tb, ub, DT, gx=gb)
    assert not np.isfinite(bad[0][2]).all() and not np.isfinite(bad[0][501]).all()  # plain floating point: inf / NaN, nothing faults
    others = ~np.isin(np.arange(N), (2, 501, 999))
    for a, b in zip(bad, clean):
        assert np.array_equal(a[..., others, :], b[..., others, :])


@pytest.mark.parametrize("name", ["iiwa14", "tree12"])
def test_generated_host_api_demo(name, tmp_path, torch_cuda, libs):
    """A hipcc-compiled downstream program calling the emitted rollout_adjoint<T> host wrappers gets what the C ABI gives (max|delta| = 0), fp32 and fp64"""
    lib = libs(name)
    n = lib.n
    Nd, S = 500, 16
    x0, u = inputs(n, Nd, S, 25)
    g = cotangent(n, Nd, S, 25)
    gen_dir = tmp_path / "gen"
    generate_header(RobotModel.from_fixture(name), str(gen_dir))
    exe = str(tmp_path / "host_api_rollout_adjoint_demo")
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "host_api_rollout_adjoint_demo.hip")
    subprocess.check_call([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + flags + ["-I" + str(gen_dir), src, "-o", exe])
    (tmp_path / "x0.bin").write_bytes(np.hstack([x0, np.zeros((Nd, n), np.float32)]).astype(np.float64).tobytes())
    (tmp_path / "u.bin").write_bytes(u.astype(np.float64).tobytes())
    (tmp_path / "gx.bin").write_bytes(g.astype(np.float64).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "x0.bin"), str(tmp_path / "u.bin"), str(tmp_path / "gx.bin"), str(Nd), str(S), repr(DT), str(tmp_path / "f32.bin"),
                                   str(tmp_path / "f64.bin")], text=True, timeout=300)
    assert out.count("Single Call ROLLOUT_ADJ") == 2 and out.count("max|delta|") == 4
    for line in out.splitlines():
        if "max|delta|" in line:
            assert float(line.split("=")[-1]) == 0.0, line
    for fname, dtype, roll, adj in (("f32.bin", np.float32, lib.rollout_host, lib.rollout_adjoint_host), ("f64.bin", np.float64, lib.rollout_host_f64, lib.rollout_adjoint_host_f64)):
        got = np.frombuffer((tmp_path / fname).read_bytes(), dtype=np.float64)
        traj = roll(x0.astype(dtype), u.astype(dtype), DT)
        ref = np.concatenate([a.astype(np.float64).reshape(-1) for a in (traj,) + adj(traj, u.astype(dtype), DT, gx=g.astype(dtype))])
        assert got.shape == ref.shape and np.abs(got - ref).max() == 0.0, fname
