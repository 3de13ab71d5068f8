"""End-effector kinematics (end_effector_pose / _gradient / _gradient_hessian) without a GPU.

1. The fp64 NumPy oracle (GRiDCodeGenerator.test_end_effector_pose*) is anchored: a 3-link planar arm in closed form, and central differences
   of pose -> gradient and gradient -> Hessian on four fixtures (a chain, a quadruped, a robot with prismatic joints, a humanoid).
2. The generated kernels, C ABI and ctypes binding run under the CPU emulation (tests/emu_harness.py) and are compared with the oracle.
"""
import ctypes

import numpy as np
import pytest

from emu_harness import emu_library
from gridcodegenerator_amd import GRiDCodeGenerator, RobotModel

TOL32, TOL64 = 1e-4, 1e-9
HIP_ERROR_INVALID_VALUE = 1  # (value of the emulated hipErrorInvalidValue)
EMU_ROBOTS = ["iiwa14", "hyq", "mixed5", "tree12", "atlas"]


def wrap(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


def oracle(gen, q):
    """(pose (N, 6E), gradient (N, 6En) in the deePos layout, Hessian (N, 6En^2) in the d2eePos layout)"""
    P = np.stack([gen.test_end_effector_pose(x).ravel() for x in q])
    G = np.stack([gen.test_end_effector_pose_gradient(x).transpose(0, 2, 1).ravel() for x in q])
    H = np.stack([gen.test_end_effector_pose_hessian(x).ravel() for x in q])
    return P, G, H


def regular(P, E):
    """solves whose end effectors all stay away from pitch = +-pi/2 (where roll and yaw are singular)"""
    return np.cos(P.reshape(P.shape[0], E, 6)[:, :, 4]).min(axis=1) >= 0.05


def rel_err(got, ref):
    got = got.reshape(got.shape[0], -1).astype(np.float64)
    ref = ref.reshape(ref.shape[0], -1)
    return (np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-30)).max()


def pose_err(got, ref):
    d = (got.astype(np.float64) - ref).reshape(got.shape[0], -1, 6)
    d[:, :, 3:] = wrap(d[:, :, 3:])
    return (np.abs(d).reshape(got.shape[0], -1).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-30)).max()


# ---------------------------------------------------------------------------------------------------- oracle anchoring
PLANAR = {"name": "planar3", "base_link": "base", "joints": [
    {"name": "j%d" % i, "type": "revolute", "axis": "z", "parent_link": "base" if i == 0 else "l%d" % (i - 1), "xyz": [0.0 if i == 0 else L, 0, 0],
     "rpy": [0, 0, 0], "link": {"name": "l%d" % i, "mass": 1.0, "com": [0.1, 0, 0], "inertia": [0.01, 0, 0, 0.01, 0, 0.01]}}
    for i, L in enumerate([0.0, 0.7, 0.45])]}


def test_oracle_planar_arm_closed_form():
    gen = GRiDCodeGenerator(RobotModel(PLANAR))
    l1, l2 = 0.7, 0.45
    for q in np.random.default_rng(3).uniform(-3, 3, (20, 3)):
        P = gen.test_end_effector_pose(q)
        assert P.shape == (1, 6)
        x = l1 * np.cos(q[0]) + l2 * np.cos(q[0] + q[1])
        y = l1 * np.sin(q[0]) + l2 * np.sin(q[0] + q[1])
        np.testing.assert_allclose(P[0, :3], [x, y, 0.0], atol=1e-12)
        assert abs(P[0, 3]) < 1e-12 and abs(P[0, 4]) < 1e-12
        assert abs(wrap(P[0, 5] - (q[0] + q[1] + q[2]))) < 1e-12


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "mixed5", "atlas"])
def test_oracle_derivatives_match_central_differences(name):
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name))
    n = gen.model.n
    rng = np.random.default_rng(11)
    h = 1e-6
    checked = 0
    for q in rng.uniform(-1.2, 1.2, (6, n)):
        P = gen.test_end_effector_pose(q)
        if np.cos(P[:, 4]).min() < 0.2:  # (away from the atan2 branch cuts)
            continue
        G, H = gen.test_end_effector_pose_gradient(q), gen.test_end_effector_pose_hessian(q)
        I = np.eye(n)
        Gfd = np.stack([wrap(gen.test_end_effector_pose(q + h * I[j]) - gen.test_end_effector_pose(q - h * I[j])) / (2 * h) for j in range(n)], axis=-1)
        Hfd = np.stack([(gen.test_end_effector_pose_gradient(q + h * I[j]) - gen.test_end_effector_pose_gradient(q - h * I[j])) / (2 * h) for j in range(n)], axis=-1)
        assert np.abs(G - Gfd).max() <= 1e-6 * max(1.0, np.abs(G).max())
        assert np.abs(H - Hfd).max() <= 1e-6 * max(1.0, np.abs(H).max())
        checked += 1
    assert checked >= 3


# ---------------------------------------------------------------------------------------------------- generated code under the CPU emulation
@pytest.fixture(scope="module")
def emu():
    libs = {}

    def get(name):
        if name not in libs:
            libs[name] = emu_library(name, max_timesteps=64)
        return libs[name]

    yield get
    for lib in libs.values():
        lib.close()


def states(n, N, seed, width):
    q = np.random.default_rng(seed).uniform(-1.5, 1.5, (N, n))
    if width == 3 * n:
        q = np.hstack([q, np.random.default_rng(seed + 1).uniform(-2, 2, (N, 2 * n))])
    return q


@pytest.mark.parametrize("name", EMU_ROBOTS)
@pytest.mark.parametrize("width", ["n", "3n"])
def test_emulated_kinematics_match_oracle(name, width, emu):
    lib = emu(name)
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name))
    n, E, N = lib.n, lib.num_end_effectors, 64
    assert lib.end_effector_joints == [j for j in range(n) if not gen.model.children[j]]
    x = states(n, N, 5, n if width == "n" else 3 * n)
    q = x[:, :n]
    P, G, H = oracle(gen, q)
    ok = regular(P, E)
    assert ok.mean() > 0.9
    p32 = lib.end_effector_pose_host(x.astype(np.float32))
    g32 = lib.end_effector_pose_gradient_host(x.astype(np.float32))
    h32, hg32 = lib.end_effector_pose_gradient_hessian_host(x.astype(np.float32))
    assert p32.shape == (N, 6 * E) and g32.shape == (N, 6 * E * n) and h32.shape == (N, 6 * E * n * n)
    assert pose_err(p32, P) <= TOL32
    assert rel_err(g32[ok], G[ok]) <= TOL32
    assert rel_err(h32[ok], H[ok]) <= TOL32
    assert np.array_equal(hg32, g32), "the Hessian kernel's deePos must be bit-identical to the gradient kernel's"
    Hs = h32.reshape(N, E, 6, n, n)
    assert np.array_equal(Hs, Hs.transpose(0, 1, 2, 4, 3)), "the Hessian must be exactly symmetric"
    # structural zeros: entries of joints off a leaf's root path
    for e, leaf in enumerate(lib.end_effector_joints):
        off = np.array([j not in gen.model.ancestors[leaf] + [leaf] for j in range(n)])
        assert (g32.reshape(N, E, n, 6)[:, e, off, :] == 0).all()
        assert (Hs[:, e][:, :, off, :] == 0).all() and (Hs[:, e][:, :, :, off] == 0).all()
    p64 = lib.host_f64("end_effector_pose", x)
    g64 = lib.host_f64("end_effector_pose_gradient", x)
    h64, hg64 = lib.host_f64("end_effector_pose_gradient_hessian", x)
    assert pose_err(p64, P) <= TOL64
    assert rel_err(g64[ok], G[ok]) <= TOL64
    assert rel_err(h64[ok], H[ok]) <= TOL64
    assert np.array_equal(hg64, g64)


def _device_run(lib, which, x, fill=np.nan, dtype=np.float32, dee=True):
    """device entry point on emulated 'device' buffers (host memory): NaN-filled outputs, input with its own stride"""
    n, E = lib.n, lib.num_end_effectors
    N = x.shape[0]
    xin = np.ascontiguousarray(x, dtype=dtype)
    cols = (6 * E, 6 * E * n, 6 * E * n * n)[which]
    out = np.full((N, cols), fill, dtype=dtype)
    g = np.full((N, 6 * E * n), fill, dtype=dtype) if (which == 2 and dee) else None
    P = lambda a: ctypes.c_void_p(None) if a is None else ctypes.c_void_p(a.ctypes.data)
    sfx = "_f64" if dtype == np.float64 else ""
    L = lib.lib
    if which == 0:
        rc = L["grid_end_effector_pose_device" + sfx](lib.handle, P(xin), ctypes.c_int(xin.shape[1]), ctypes.c_int(N), P(out), ctypes.c_void_p(None))
    elif which == 1:
        rc = L["grid_end_effector_pose_gradient_device" + sfx](lib.handle, P(xin), ctypes.c_int(xin.shape[1]), ctypes.c_int(N), P(out), ctypes.c_void_p(None))
    else:
        rc = L["grid_end_effector_pose_gradient_hessian_device" + sfx](lib.handle, P(xin), ctypes.c_int(xin.shape[1]), ctypes.c_int(N), P(out), P(g), ctypes.c_void_p(None))
    return rc, out, g


@pytest.mark.parametrize("name", ["iiwa14", "hyq", "atlas"])
def test_emulated_device_form_equals_host_form_and_overwrites_nan(name, emu):
    lib = emu(name)
    n = lib.n
    x = states(n, 37, 9, 3 * n)  # (a batch that leaves lane groups of the last block idle)
    for dtype in (np.float32, np.float64):
        host = [lib._ee_host(0, x, dtype), lib._ee_host(1, x, dtype)] + list(lib._ee_host(2, x, dtype))
        rc0, p, _ = _device_run(lib, 0, x, dtype=dtype)
        rc1, g, _ = _device_run(lib, 1, x, dtype=dtype)
        rc2, h, hg = _device_run(lib, 2, x, dtype=dtype)
        assert rc0 == rc1 == rc2 == 0
        for got, ref in zip([p, g, h, hg], host):
            assert not np.isnan(got).any(), "every output element must be written"
            assert np.array_equal(got, ref)
        rc, h2, none = _device_run(lib, 2, x, dtype=dtype, dee=False)  # (d_deePos may be NULL)
        assert rc == 0 and none is None and np.array_equal(h2, h)


def test_emulated_launch_dims_grid_stride(emu):
    lib = emu("iiwa14")
    n = lib.n
    x = states(n, 50, 4, n)
    ref = [lib.end_effector_pose_host(x.astype(np.float32)), lib.end_effector_pose_gradient_hessian_host(x.astype(np.float32))[0]]
    lib.set_launch_dims(blocks=2, threads=32)  # (few blocks: every lane group walks the batch)
    try:
        got = [_device_run(lib, 0, x)[1], _device_run(lib, 2, x)[1]]
    finally:
        lib.set_launch_dims(0, 0)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_emulated_boundary_cases(emu):
    lib = emu("hyq")
    L, H, n = lib.lib, lib.handle, lib.n
    E = lib.num_end_effectors
    q = np.zeros((4, n), dtype=np.float32)
    out = np.zeros((4, 6 * E * n * n), dtype=np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    NULL = ctypes.c_void_p(None)
    for fn in ("grid_end_effector_pose_device", "grid_end_effector_pose_gradient_device"):
        f = L[fn]
        assert f(H, NULL, n, 4, P(out), NULL) == HIP_ERROR_INVALID_VALUE
        assert f(H, P(q), n, 4, NULL, NULL) == HIP_ERROR_INVALID_VALUE
        assert f(H, P(q), n - 1, 4, P(out), NULL) == HIP_ERROR_INVALID_VALUE
        assert f(H, P(q), n, -1, P(out), NULL) == HIP_ERROR_INVALID_VALUE
        assert f(NULL, P(q), n, 4, P(out), NULL) == HIP_ERROR_INVALID_VALUE
        assert f(H, NULL, n, 0, NULL, NULL) == 0  # (an empty batch touches nothing)
    f = L.grid_end_effector_pose_gradient_hessian_device
    assert f(H, P(q), n, 4, NULL, NULL, NULL) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n - 1, 4, P(out), NULL, NULL) == HIP_ERROR_INVALID_VALUE
    for fn in ("grid_end_effector_pose_host", "grid_end_effector_pose_gradient_host"):
        f = L[fn]
        assert f(H, NULL, n, 4, P(out)) == HIP_ERROR_INVALID_VALUE
        assert f(H, P(q), n, 4, NULL) == HIP_ERROR_INVALID_VALUE
        assert f(H, P(q), n - 1, 4, P(out)) == HIP_ERROR_INVALID_VALUE
        assert f(H, P(q), n, -3, P(out)) == HIP_ERROR_INVALID_VALUE
        assert f(H, P(q), n, lib.max_timesteps + 1, P(out)) == HIP_ERROR_INVALID_VALUE
    f = L.grid_end_effector_pose_gradient_hessian_host
    assert f(H, P(q), n, lib.max_timesteps + 1, P(out), NULL) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n, 4, NULL, NULL) == HIP_ERROR_INVALID_VALUE
    assert L.grid_end_effector_joints(NULL) == HIP_ERROR_INVALID_VALUE
    # the handle still works after the rejected calls
    assert lib.end_effector_pose_host(q).shape == (4, 6 * E)


# ---------------------------------------------------------------------------------------------------- emitted surface
def test_emitted_surface(tmp_path):
    import os

    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        src = GRiDCodeGenerator(RobotModel.from_fixture("hyq")).gen_all_code()
    finally:
        os.chdir(cwd)
    for name in ("end_effector_pose", "end_effector_pose_gradient", "end_effector_pose_gradient_hessian"):
        for sfx in ("_inner", "_device", "_kernel", "", "_single_timing", "_compute_only"):
            assert ("void %s%s(" % (name, sfx)) in src, name + sfx
    for c in ("EE_POS", "DEE_POS", "D2EE_POS"):
        for k in ("LDS_PER_SOLVE", "OUT_PER_SOLVE", "SUGGESTED_THREADS", "DYNAMIC_SHARED_MEM_COUNT"):
            assert "const int %s_%s = " % (c, k) in src
    init = src[src.index("gridData<T> *init_gridData(int NUM_TIMESTEPS){"):]
    init = init[:init.index("return hd_data;")]
    for nm in ("eePos", "deePos", "d2eePos"):
        assert "hd_data->d_%s = nullptr;" % nm in init and "hd_data->h_%s = nullptr;" % nm in init
    assert src.count("void end_effector_pose_kernel(") == 1  # (the nested `wide` library does not repeat them)
    assert "__syncthreads" not in src.split("end-effector kinematics (end_effector_pose")[1]
    for name in ("gen_end_effector_pose_inner", "gen_end_effector_pose_device", "gen_end_effector_pose_kernel", "gen_end_effector_pose_host",
                 "gen_end_effector_pose_gradient_hessian_host", "gen_end_effector_pose_inner_temp_mem_size", "gen_eepose_and_derivatives"):
        assert hasattr(GRiDCodeGenerator, name)
