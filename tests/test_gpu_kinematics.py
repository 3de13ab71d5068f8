"""End-effector kinematics on the GPU (run with -m gpu on an MI355X), through the C ABI (include/grid_capi.h) as in test_gpu_parity.py.

Acceptance: per solve max|delta| <= 1e-4 * max|reference| for the fp32 kernels against the fp64 oracle (GRiDCodeGenerator.test_end_effector_pose*),
1e-9 for the fp64 instantiations.  Angles are compared as wrapped differences; derivative comparisons skip states where an end effector is within
cos(pitch) < 0.05 of the roll/yaw singularity (fewer than 2 % of the states are skipped).  The fp64 NumPy Hessian oracle costs ~40 ms per humanoid
state, so the Hessian is checked on the first 256 of the 4 096 states; pose and gradient on all of them.
"""
import ctypes

import numpy as np
import pytest

from gridcodegenerator_amd import GRiDCodeGenerator, RobotModel
from gridcodegenerator_amd._test import _ee_all
from gridcodegenerator_amd.runtime import GridLibrary, build_library

pytestmark = pytest.mark.gpu
TOL32, TOL64 = 1e-4, 1e-9
ROBOTS = ["iiwa14", "hyq", "atlas", "mixed5", "arm6", "chain12", "chain8", "tree12"]


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
            cache[name] = GridLibrary(build_library(name), device=0, max_timesteps=8192)  # raises when the HIP .so is missing
        return cache[name]

    yield get
    for lib in cache.values():
        lib.close()


def wrap(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


def states(n, N, seed):
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, (N, n))


def oracle(gen, q, order):
    out = [_ee_all(gen, x, order) for x in q]
    P = np.stack([o[0].ravel() for o in out])
    G = np.stack([o[1].transpose(0, 2, 1).ravel() for o in out])
    H = np.stack([o[2].ravel() for o in out]) if order == 2 else None
    return P, G, H


def regular(P, E):
    return np.cos(P.reshape(P.shape[0], E, 6)[:, :, 4]).min(axis=1) >= 0.05


def rel_err(got, ref):
    got = got.reshape(got.shape[0], -1).astype(np.float64)
    ref = ref.reshape(ref.shape[0], -1)
    return (np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-30)).max()


def pose_err(got, ref):
    d = (got.astype(np.float64) - ref).reshape(got.shape[0], -1, 6)
    d[:, :, 3:] = wrap(d[:, :, 3:])
    return (np.abs(d).reshape(got.shape[0], -1).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-30)).max()


def run(torch, lib, x, dtype=None, dee=True):
    """the three device entry points on NaN-filled outputs; returns (pose, gradient, Hessian, Hessian kernel's gradient) as NumPy arrays"""
    dtype = dtype or torch.float32
    n, E = lib.n, lib.num_end_effectors
    N = x.shape[0]
    d_q = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()
    nan = lambda c: torch.full((N, c), float("nan"), dtype=dtype, device="cuda")
    p, g, h = nan(6 * E), nan(6 * E * n), nan(6 * E * n * n)
    hg = nan(6 * E * n) if dee else None
    s = torch.cuda.current_stream().cuda_stream
    if dtype == torch.float32:
        lib.end_effector_pose_device(d_q, N, p, stride=x.shape[1], stream=s)
        lib.end_effector_pose_gradient_device(d_q, N, g, stride=x.shape[1], stream=s)
        lib.end_effector_pose_gradient_hessian_device(d_q, N, h, hg, stride=x.shape[1], stream=s)
    else:
        P = lambda t: ctypes.c_void_p(None) if t is None else ctypes.c_void_p(t.data_ptr())
        L, H, st, cN, sv = lib.lib, lib.handle, ctypes.c_int(x.shape[1]), ctypes.c_int(N), ctypes.c_void_p(s)
        lib._check(L.grid_end_effector_pose_device_f64(H, P(d_q), st, cN, P(p), sv))
        lib._check(L.grid_end_effector_pose_gradient_device_f64(H, P(d_q), st, cN, P(g), sv))
        lib._check(L.grid_end_effector_pose_gradient_hessian_device_f64(H, P(d_q), st, cN, P(h), P(hg), sv))
    torch.cuda.synchronize()
    return [t.cpu().numpy() if t is not None else None for t in (p, g, h, hg)]


@pytest.mark.parametrize("name", ROBOTS)
def test_kinematics_fp32_match_oracle(name, torch_cuda, libs):
    lib = libs(name)
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name))
    n, E = lib.n, lib.num_end_effectors
    q = states(n, 4096, 2024)
    x = np.hstack([q, np.random.default_rng(7).uniform(-2, 2, (4096, 2 * n))])  # (q_qd_u rows: stride 3n)
    p, g, h, hg = run(torch_cuda, lib, x.astype(np.float32))
    for a in (p, g, h, hg):
        assert not np.isnan(a).any(), "every output element must be written"
    P, G, _ = oracle(gen, q, 1)
    ok = regular(P, E)
    assert 1 - ok.mean() < 0.02, "%.1f %% of the states skipped" % (100 * (1 - ok.mean()))
    assert pose_err(p, P) <= TOL32
    assert rel_err(g[ok], G[ok]) <= TOL32
    assert np.array_equal(hg, g), "the Hessian kernel's deePos must be bit-identical to the gradient kernel's"
    Hs = h.reshape(-1, E, 6, n, n)
    assert np.array_equal(Hs, Hs.transpose(0, 1, 2, 4, 3)), "the Hessian must be exactly symmetric"
    m = 256
    _, _, Hr = oracle(gen, q[:m], 2)
    assert rel_err(h[:m][ok[:m]], Hr[ok[:m]]) <= TOL32
    for e, leaf in enumerate(lib.end_effector_joints):
        off = np.array([j not in gen.model.ancestors[leaf] + [leaf] for j in range(n)])
        assert (g.reshape(-1, E, n, 6)[:, e, off, :] == 0).all()
        assert (Hs[:, e][:, :, off, :] == 0).all()


@pytest.mark.parametrize("name", ROBOTS)
def test_kinematics_fp64_match_oracle(name, torch_cuda, libs):
    lib = libs(name)
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name))
    n, E = lib.n, lib.num_end_effectors
    q = states(n, 256, 99)
    p, g, h, hg = run(torch_cuda, lib, q, dtype=torch_cuda.float64)
    P, G, H = oracle(gen, q, 2)
    ok = regular(P, E)
    assert pose_err(p, P) <= TOL64
    assert rel_err(g[ok], G[ok]) <= TOL64
    assert rel_err(h[ok], H[ok]) <= TOL64
    assert np.array_equal(hg, g)


@pytest.mark.parametrize("blocks", [0, 7])
def test_kinematics_batch_sizes_and_launch_dims(blocks, torch_cuda, libs):
    """N = 1, 4 099 and 65 536 on the 7-DoF arm: the default grid and 7 blocks (every lane group grid-strides; tail lane groups idle)"""
    lib = libs("iiwa14")
    gen = GRiDCodeGenerator(RobotModel.from_fixture("iiwa14"))
    n = lib.n
    big = states(n, 65536, 5).astype(np.float32)
    lib.set_launch_dims(0, 0)
    ref = run(torch_cuda, lib, big)
    P, G, H = oracle(gen, big[:64].astype(np.float64), 2)
    ok = regular(P, 1)
    assert pose_err(ref[0][:64], P) <= TOL32 and rel_err(ref[1][:64][ok], G[ok]) <= TOL32 and rel_err(ref[2][:64][ok], H[ok]) <= TOL32
    lib.set_launch_dims(blocks, 0)
    try:
        for N in (1, 4099, 65536):
            got = run(torch_cuda, lib, big[:N])
            for a, b in zip(got, ref):
                assert not np.isnan(a).any()
                assert np.array_equal(a, b[:N])
    finally:
        lib.set_launch_dims(0, 0)


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "atlas", "mixed5"])
def test_kinematics_host_equals_device(name, torch_cuda, libs):
    lib = libs(name)
    n = lib.n
    q = states(n, 3000, 17).astype(np.float32)
    dev = run(torch_cuda, lib, q)
    host = [lib.end_effector_pose_host(q), lib.end_effector_pose_gradient_host(q)] + list(lib.end_effector_pose_gradient_hessian_host(q))
    for a, b in zip(dev, host):
        assert np.array_equal(a, b)
    q64 = q[:200].astype(np.float64)
    dev64 = run(torch_cuda, lib, q64, dtype=torch_cuda.float64)
    host64 = [lib.host_f64("end_effector_pose", q64), lib.host_f64("end_effector_pose_gradient", q64)] + list(lib.host_f64("end_effector_pose_gradient_hessian", q64))
    for a, b in zip(dev64, host64):
        assert np.array_equal(a, b)
