"""Joint-space inertia matrix M(q) on the GPU (run with -m gpu on an MI355X), through the C ABI (include/grid_capi.h) as in test_gpu_parity.py.

Acceptance: per solve max|delta| <= 1e-4 * max|M| for the fp32 kernel against the fp64 oracle (GRiDCodeGenerator.test_crba), 1e-9 for the fp64
instantiation; exact symmetry and exact structural zeros.  M is tied to the other kernels of the same library: M direct_minv = I and
M FD(q, qd, u) + ID(q, qd, 0) = u in fp64, damping included.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gridcodegenerator_amd import GRiDCodeGenerator, RobotModel
from gridcodegenerator_amd.runtime import HIPCC_FLAGS, GridLibrary, build_library, generate_header

pytestmark = pytest.mark.gpu
TOL32, TOL64 = 1e-4, 1e-9
ROBOTS = ["iiwa14", "hyq", "atlas", "mixed5", "arm6", "chain12", "chain8", "tree12"]
N = 4096


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
            cache[name] = GridLibrary(build_library(name), device=0, max_timesteps=N)  # raises when the HIP .so is missing
        return cache[name]

    yield get
    for lib in cache.values():
        lib.close()


def inputs(n, seed):
    rng = np.random.default_rng(seed)
    return np.hstack([rng.uniform(-np.pi, np.pi, (N, n)), rng.uniform(-2, 2, (N, n)), rng.uniform(-5, 5, (N, n))])


def unrelated(m):
    n = m.n
    rel = np.eye(n, dtype=bool)
    for j in range(n):
        for a in m.ancestors[j]:
            rel[a, j] = rel[j, a] = True
    return ~rel


def rel_err(got, ref):
    got = got.reshape(got.shape[0], -1).astype(np.float64)
    ref = ref.reshape(ref.shape[0], -1)
    return (np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max()


@pytest.mark.parametrize("name", ROBOTS)
def test_crba_matches_oracle(name, torch_cuda, libs):
    lib = libs(name)
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name))
    n = lib.n
    x = inputs(n, 3)
    ref = np.stack([gen.test_crba(q).ravel() for q in x[:, :n]])
    zero = unrelated(gen.model)
    for width in (n, 3 * n):
        m32 = lib.crba_host(x[:, :width].astype(np.float32))
        m64 = lib.host_f64("crba", x[:, :width])
        assert rel_err(m32, ref) <= TOL32
        assert rel_err(m64, ref) <= TOL64
        for M in (m32, m64):
            Ms = M.reshape(N, n, n)
            assert np.array_equal(Ms, Ms.transpose(0, 2, 1)), "M must be exactly symmetric"
            assert (Ms[:, zero] == 0).all(), "pairs where neither joint is an ancestor of the other must be exact zeros"
    # every M is positive definite (the fp32 record itself)
    np.linalg.cholesky(m32.reshape(N, n, n).astype(np.float64))


@pytest.mark.parametrize("name", ROBOTS)
def test_crba_device_form(name, torch_cuda, libs):
    torch = torch_cuda
    lib = libs(name)
    n = lib.n
    x = inputs(n, 4).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    d_M = torch.full((N, n * n), float("nan"), dtype=torch.float32, device="cuda")
    lib.crba_device(d_x, N, d_M, stride=3 * n)
    torch.cuda.synchronize()
    got = d_M.cpu().numpy()
    assert not np.isnan(got).any(), "every output element must be written"
    assert np.array_equal(got, lib.crba_host(x))


@pytest.mark.parametrize("name", ROBOTS)
def test_crba_consistent_with_minv_fd_and_id(name, torch_cuda, libs):
    lib = libs(name)
    n = lib.n
    x = inputs(n, 5)
    M = lib.host_f64("crba", x).reshape(N, n, n)
    A = lib.host_f64("direct_minv", x).reshape(N, n, n).transpose(0, 2, 1)  # (upper triangle, column-major)
    Minv = np.triu(A) + np.transpose(np.triu(A, 1), (0, 2, 1))
    assert np.abs(M @ Minv - np.eye(n)).max() <= 1e-8
    u = x[:, 2 * n:]
    qdd = lib.host_f64("forward_dynamics", x)
    c = lib.host_f64("inverse_dynamics", x[:, :2 * n])  # (q, qd, qdd = 0): bias forces, gravity and damping included
    res = np.einsum("kij,kj->ki", M, qdd) + c - u
    assert np.abs(res).max() <= 1e-8 * np.abs(u).max()


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "atlas", "mixed5"])
def test_generated_host_api_crba(name, torch_cuda, libs, tmp_path):
    """a reference-style driver: init_gridData -> crba -> crba_single_timing (3 repetitions) -> crba_compute_only -> close_grid, float and double"""
    lib = libs(name)
    n = lib.n
    Nd = 512
    x = inputs(n, 6)[:Nd]
    gen_dir = tmp_path / "gen"
    generate_header(RobotModel.from_fixture(name), str(gen_dir))
    exe = str(tmp_path / "host_api_crba_demo")
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "host_api_crba_demo.hip")
    subprocess.check_call([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + flags + ["-I" + str(gen_dir), src, "-o", exe])
    (tmp_path / "in.bin").write_bytes(x.astype(np.float64).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin"), str(Nd), str(tmp_path / "f32.bin"), str(tmp_path / "f64.bin")], text=True, timeout=300)
    assert "Single Call CRBA" in out
    for line in out.splitlines():
        if "max|delta|" in line:
            assert float(line.split("=")[-1]) == 0.0, line
    f32 = np.frombuffer((tmp_path / "f32.bin").read_bytes(), dtype=np.float64).reshape(Nd, -1)
    f64 = np.frombuffer((tmp_path / "f64.bin").read_bytes(), dtype=np.float64).reshape(Nd, -1)
    assert np.array_equal(f32, lib.crba_host(x.astype(np.float32)).astype(np.float64))
    assert np.array_equal(f64, lib.host_f64("crba", x))
