"""Fused multi-step rollout on the GPU (run with -m gpu on an MI355X), through the C ABI (include/grid_capi.h) and the ctypes binding.

Reference: tests/rollout_reference.py, the fp64 oracle stepped in NumPy fp64.  Metric: per solve max|got - ref| / max(1, max|ref|) over everything the
solve owns.  Bar: 1e-4 for the fp32 kernel (the project's acceptance for every fp32 kernel), 1e-9 for the fp64 twin.  Inputs q0, qd0 ~ U(-1, 1),
u ~ U(-5, 5), dt = 1e-3: over 64 steps the fp32 oracle alone stays below 1e-6 of the fp64 one (dt = 1e-2 diverges with these torques and is not used).
Every solve and every step is compared; NaN on either side fails.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gridcodegenerator_amd import RobotModel
from gridcodegenerator_amd.runtime import HIPCC_FLAGS, GridLibrary, build_library, generate_header
from rollout_reference import FIXTURES, TOL32, TOL64, inputs, oracle_rollout, per_solve_err

pytestmark = pytest.mark.gpu
T, DT = 64, 1e-3
MAX_N = 16384


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
    print("[rollout parity] %s: worst %.3g, p99.9 %.3g over %d solves" % (tag, err.max(), np.quantile(err, 0.999), err.size))


@pytest.mark.parametrize("name", FIXTURES)
def test_rollout_matches_the_oracle(name, torch_cuda, libs):
    """N = 1000 (a partial last block), every solve, every step; fp32 and the fp64 twin"""
    lib = libs(name)
    N = 1000
    x0, u = inputs(lib.n, N, T, 21)
    ref = oracle_rollout(name, x0, u, DT)
    traj = lib.rollout_host(x0, u, DT)
    assert np.array_equal(traj[0], x0)
    err = per_solve_err(traj, ref)
    report(name + " fp32", err)
    assert err.max() <= TOL32
    xT = lib.rollout_host(x0, u, DT, final_only=True)
    assert np.array_equal(xT, traj[T])
    err64 = per_solve_err(lib.rollout_host_f64(x0.astype(np.float64), u.astype(np.float64), DT), ref)
    report(name + " fp64", err64)
    assert err64.max() <= TOL64


@pytest.mark.parametrize("name,N", [("iiwa14", 16384), ("hyq", 4096)])
def test_rollout_at_the_configured_batches(name, N, torch_cuda, libs):
    """BASELINE.json's batches, xT only, every solve checked"""
    torch = torch_cuda
    lib = libs(name)
    n = lib.n
    x0, u = inputs(n, N, T, 22)
    d_x0, d_u = torch.from_numpy(x0).cuda(), torch.from_numpy(u).cuda()
    d_xT = torch.zeros((N, 2 * n), dtype=torch.float32, device="cuda")
    lib.rollout_device(d_x0, d_u, N, T, DT, d_xT=d_xT, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = per_solve_err(d_xT.cpu().numpy(), oracle_rollout(name, x0, u, DT, final_only=True))
    report("%s @%d xT" % (name, N), err)
    assert err.max() <= TOL32


@pytest.mark.parametrize("name", ["iiwa14", "atlas"])
def test_torch_tensors_on_a_side_stream_modes_and_composition(name, torch_cuda, libs):
    torch = torch_cuda
    lib = libs(name)
    n = lib.n
    N = 1000
    x0, u = inputs(n, N, T, 23)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_x0 = torch.from_numpy(np.hstack([x0, np.zeros((N, n), np.float32)])).cuda()  # (N, 3n) rows as they are
        d_u = torch.from_numpy(u).cuda()
        d_traj = torch.zeros((T + 1, N, 2 * n), dtype=torch.float32, device="cuda")
        d_xT, d_xT_only, d_mid, d_end = (torch.zeros((N, 2 * n), dtype=torch.float32, device="cuda") for _ in range(4))
        s = side.cuda_stream
        lib.rollout_device(d_x0, d_u, N, T, DT, d_traj=d_traj, d_xT=d_xT, stride_x0=3 * n, stream=s)
        lib.rollout_device(d_x0, d_u, N, T, DT, d_xT=d_xT_only, stride_x0=3 * n, stream=s)
        # composition: 24 steps, then 40 more from that state
        lib.rollout_device(d_x0, d_u, N, 24, DT, d_xT=d_mid, stride_x0=3 * n, stream=s)
        lib.rollout_device(d_mid, d_u[24:], N, T - 24, DT, d_xT=d_end, stream=s)
    side.synchronize()
    assert torch.equal(d_traj[0], d_x0[:, :2 * n])
    assert torch.equal(d_traj[T], d_xT) and torch.equal(d_xT, d_xT_only)
    assert torch.equal(d_traj[24], d_mid) and torch.equal(d_end, d_xT)
    assert np.array_equal(d_traj.cpu().numpy(), lib.rollout_host(x0, u, DT))
    # one control sequence for all solves
    with torch.cuda.stream(side):
        d_shared = d_u[:, 0].contiguous()
        d_tiled = d_shared[:, None, :].expand(T, N, n).contiguous()
        a, b = torch.zeros_like(d_xT), torch.zeros_like(d_xT)
        lib.rollout_device(d_x0, d_shared, N, T, DT, d_xT=a, stride_x0=3 * n, u_shared=True, stream=side.cuda_stream)
        lib.rollout_device(d_x0, d_tiled, N, T, DT, d_xT=b, stride_x0=3 * n, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["iiwa14", "hyq"])
def test_one_launch_equals_T_aba_launches(name, torch_cuda, libs):
    """What a user did before: T launches of aba_device with a torch fp32 update in between.  The kernel may contract qd + dt*qdd to an FMA, so the two
    agree to the error bar, not bit for bit."""
    torch = torch_cuda
    lib = libs(name)
    n = lib.n
    N = 1000
    x0, u = inputs(n, N, T, 24)
    st = torch.cuda.current_stream().cuda_stream
    d_x = torch.from_numpy(np.hstack([x0, u[0]])).cuda()  # (N, 3n): q | qd | u_t
    d_u = torch.from_numpy(u).cuda()
    d_qdd = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    d_xT = torch.zeros((N, 2 * n), dtype=torch.float32, device="cuda")
    lib.rollout_device(d_x, d_u, N, T, DT, d_xT=d_xT, stride_x0=3 * n, stream=st)
    for t in range(T):
        d_x[:, 2 * n:] = d_u[t]
        lib.aba_device(d_x, N, d_qdd, stream=st)
        d_x[:, n:2 * n] += DT * d_qdd
        d_x[:, :n] += DT * d_x[:, n:2 * n]
    torch.cuda.synchronize()
    err = per_solve_err(d_xT.cpu().numpy(), d_x[:, :2 * n].cpu().numpy().astype(np.float64))
    report(name + " fused vs stepwise", err)
    assert err.max() <= TOL32


@pytest.mark.parametrize("name", ["iiwa14", "hyq"])
def test_generated_host_api_demo(name, tmp_path, torch_cuda, libs):
    """A hipcc-compiled downstream program calling the emitted rollout<T> host wrappers gets what the C ABI gives"""
    lib = libs(name)
    n = lib.n
    Nd, S = 500, 16
    x0, u = inputs(n, Nd, S, 25)
    gen_dir = tmp_path / "gen"
    generate_header(RobotModel.from_fixture(name), str(gen_dir))
    exe = str(tmp_path / "host_api_rollout_demo")
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "host_api_rollout_demo.hip")
    subprocess.check_call([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + flags + ["-I" + str(gen_dir), src, "-o", exe])
    (tmp_path / "x0.bin").write_bytes(np.hstack([x0, np.zeros((Nd, n), np.float32)]).astype(np.float64).tobytes())
    (tmp_path / "u.bin").write_bytes(u.astype(np.float64).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "x0.bin"), str(tmp_path / "u.bin"), str(Nd), str(S), repr(DT), str(tmp_path / "f32.bin"), str(tmp_path / "f64.bin")],
                                  text=True, timeout=300)
    assert "Single Call ROLLOUT" in out
    for line in out.splitlines():
        if "max|delta|" in line:
            assert float(line.split("=")[-1]) == 0.0, line
    f32 = np.frombuffer((tmp_path / "f32.bin").read_bytes(), dtype=np.float64).reshape(S + 1, Nd, 2 * n)
    f64 = np.frombuffer((tmp_path / "f64.bin").read_bytes(), dtype=np.float64).reshape(S + 1, Nd, 2 * n)
    assert np.array_equal(f32, lib.rollout_host(x0, u, DT).astype(np.float64))
    assert np.array_equal(f64, lib.rollout_host_f64(x0.astype(np.float64), u.astype(np.float64), DT))
