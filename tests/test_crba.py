"""Joint-space inertia matrix M(q) (crba) without a GPU.

1. The fp64 NumPy oracle (GRiDCodeGenerator.test_crba) is anchored: a planar 2-link arm in closed form, inv(test_minv), the columns of
   RNEA(q, 0, e_j, g = 0), and inv(golden Minv) recorded from the reference.
2. The generated kernel, C ABI and ctypes binding run under the CPU emulation (tests/emu_harness.py) and are compared with the oracle.
"""
import ctypes
import glob
import os

import numpy as np
import pytest

from emu_harness import emu_library
from gridcodegenerator_amd import GRiDCodeGenerator, RobotModel
from gridcodegenerator_amd.algorithms._crba import CRBA_TIP_MAX_L
from gridcodegenerator_amd.runtime import generate_header
from test_generated_emulation import _random_tree_description

TOL32, TOL64 = 1e-4, 1e-9
HIP_ERROR_INVALID_VALUE = 1  # (value of the emulated hipErrorInvalidValue)
FIXTURES = ["iiwa14", "arm6", "chain8", "chain12", "hyq", "mixed5", "tree12", "atlas"]
HERE = os.path.dirname(os.path.abspath(__file__))


def rnd_tree(seed, n, prismatic=()):
    desc = _random_tree_description(seed, n)
    for j in prismatic:
        desc["joints"][j]["type"] = "prismatic"
    desc["name"] = desc["name"] + ("p" if prismatic else "")
    return RobotModel(desc)


# robot -> the crba inner its library must emit (the formulation direct_minv uses): all three forms are covered
EMU_ROBOTS = {"iiwa14": "crba_inner_tip", "hyq": "crba_inner_tip", "mixed5": "crba_inner", "tree12": "crba_inner_branch", "atlas": "crba_inner_branch",
              "rnd16": "crba_inner_branch", "rnd13p": "crba_inner"}
INNERS = ("crba_inner_tip", "crba_inner_branch", "crba_inner")


def robot(name):
    if name == "rnd16":
        return rnd_tree(16, 8)
    if name == "rnd13p":
        return rnd_tree(13, 7, prismatic=(1, 4, 6))
    return RobotModel.from_fixture(name)


def unrelated(m):
    """(n, n) mask of the pairs where neither joint is an ancestor of the other"""
    n = m.n
    rel = np.eye(n, dtype=bool)
    for j in range(n):
        for a in m.ancestors[j]:
            rel[a, j] = rel[j, a] = True
    return ~rel


# ---------------------------------------------------------------------------------------------------- oracle anchoring
PLANAR = {"name": "planar2", "base_link": "base", "joints": [
    {"name": "j%d" % i, "type": "revolute", "axis": "z", "parent_link": "base" if i == 0 else "l0", "xyz": [0.0 if i == 0 else 0.8, 0, 0],
     "rpy": [0, 0, 0], "link": {"name": "l%d" % i, "mass": m_, "com": [c_, 0, 0], "inertia": [0.01, 0, 0, 0.01, 0, iz]}}
    for i, (m_, c_, iz) in enumerate([(2.0, 0.35, 0.05), (1.2, 0.3, 0.02)])]}


def test_oracle_planar_arm_closed_form():
    gen = GRiDCodeGenerator(RobotModel(PLANAR))
    m1, r1, I1, m2, r2, I2, l1 = 2.0, 0.35, 0.05, 1.2, 0.3, 0.02, 0.8
    for q in np.random.default_rng(7).uniform(-3, 3, (20, 2)):
        c2 = np.cos(q[1])
        # textbook form; I1, I2 are the link inertias about the joint axis at the centre of mass
        m11 = I1 + m1 * r1 ** 2 + I2 + m2 * (l1 ** 2 + r2 ** 2 + 2 * l1 * r2 * c2)
        m12 = I2 + m2 * (r2 ** 2 + l1 * r2 * c2)
        m22 = I2 + m2 * r2 ** 2
        assert np.allclose(gen.test_crba(q), [[m11, m12], [m12, m22]], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_minv_and_rnea_columns(name):
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name))
    n = gen.model.n
    for q in np.random.default_rng(11).uniform(-2, 2, (4, n)):
        M = gen.test_crba(q)
        assert np.abs(M - np.linalg.inv(gen.test_minv(q))).max() <= 1e-10 * max(1.0, np.abs(M).max())
        zero = np.zeros(n)
        R = np.stack([gen.test_rnea(q, zero, np.eye(n)[j], GRAVITY=0.0)[0] for j in range(n)], axis=1)
        assert np.abs(M - R).max() <= 1e-10 * max(1.0, np.abs(M).max())
        assert np.array_equal(M, M.T)
        assert (M[unrelated(gen.model)] == 0).all()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(HERE, "golden", "*.npz"))))
def test_oracle_matches_reference_goldens(path):
    d = np.load(path)
    name = os.path.basename(path)[:-4]
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name.replace("_nodamp", "")))
    for q, Minv in zip(d["q"], d["Minv"]):
        M = gen.test_crba(q)
        ref = np.linalg.inv(Minv)
        assert np.abs(M - ref).max() <= 1e-9 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------- generated code under the CPU emulation
@pytest.fixture(scope="module")
def emu():
    libs = {}

    def get(name):
        if name not in libs:
            libs[name] = emu_library(robot(name), max_timesteps=64)
        return libs[name]

    yield get
    for lib in libs.values():
        lib.close()


def states(n, N, seed, width):
    q = np.random.default_rng(seed).uniform(-1.5, 1.5, (N, n))
    if width == 3 * n:
        q = np.hstack([q, np.random.default_rng(seed + 1).uniform(-2, 2, (N, 2 * n))])
    return q


def rel_err(got, ref):
    got = got.reshape(got.shape[0], -1).astype(np.float64)
    ref = ref.reshape(ref.shape[0], -1)
    return (np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max()


def emitted_inner(r, tmp_path):
    """the crba inner crba_device calls in the generated header, and whether that inner is defined there"""
    src = open(generate_header(r, str(tmp_path / r.name))).read()
    dev = src[src.index("void crba_device("):]
    dev = dev[:dev.index("\n    }\n")]  # (end of the function, one level inside the namespace)
    called = [f for f in INNERS if (f + "<T>(") in dev]
    assert len(called) == 1, called
    return called[0], ("void %s(" % called[0]) in src


@pytest.mark.parametrize("name", list(EMU_ROBOTS) + ["chain8", "chain12"])
def test_crba_inner_follows_the_direct_minv_formulation(name, tmp_path):
    r = robot(name)
    gen = GRiDCodeGenerator(r)
    # tip-frame chains up to CRBA_TIP_MAX_L joints (longer ones spill in fp64 on that form), branch-component robots, else the column walk
    want = "crba_inner_tip" if (gen.tip_frame and gen.tip_L <= CRBA_TIP_MAX_L) else ("crba_inner_branch" if gen.branch_components else "crba_inner")
    assert EMU_ROBOTS.get(name, "crba_inner") == want  # (chain8, chain12: tip-frame chains longer than CRBA_TIP_MAX_L)
    assert emitted_inner(r, tmp_path) == (want, True)


@pytest.mark.parametrize("name", list(EMU_ROBOTS))
@pytest.mark.parametrize("width", ["n", "3n"])
def test_emulated_crba_matches_oracle(name, width, emu):
    r = robot(name)
    gen = GRiDCodeGenerator(r)
    if name == "rnd13p":
        assert any(s_ >= 3 for s_ in gen.model.S_index), "the random tree must have prismatic joints"
    lib = emu(name)
    n, N = lib.n, 40
    x = states(n, N, 5, n if width == "n" else 3 * n)
    ref = np.stack([gen.test_crba(q).ravel() for q in x[:, :n]])
    zero = unrelated(gen.model)
    for dtype, tol in ((np.float32, TOL32), (np.float64, TOL64)):
        got = lib.crba_host(x) if dtype == np.float32 else lib.host_f64("crba", x)
        assert got.shape == (N, n * n) and got.dtype == dtype
        assert rel_err(got, ref) <= tol
        Ms = got.reshape(N, n, n)
        assert np.array_equal(Ms, Ms.transpose(0, 2, 1)), "M must be exactly symmetric"
        assert (Ms[:, zero] == 0).all(), "pairs where neither joint is an ancestor of the other must be exact zeros"


def _device_run(lib, x, dtype=np.float32):
    """device entry point on emulated 'device' buffers (host memory): NaN-filled output, input with its own stride"""
    n, N = lib.n, x.shape[0]
    xin = np.ascontiguousarray(x, dtype=dtype)
    out = np.full((N, n * n), np.nan, dtype=dtype)
    fn = lib.lib["grid_crba_device" + ("_f64" if dtype == np.float64 else "")]
    rc = fn(lib.handle, ctypes.c_void_p(xin.ctypes.data), ctypes.c_int(xin.shape[1]), ctypes.c_int(N), ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(None))
    return rc, out


@pytest.mark.parametrize("name", ["iiwa14", "mixed5", "atlas"])
def test_emulated_device_form_equals_host_form_and_overwrites_nan(name, emu):
    lib = emu(name)
    n = lib.n
    for width in (n, 2 * n, 3 * n):
        x = states(n, 37, 9, 3 * n)[:, :width]  # (a batch that leaves lane groups of the last block idle)
        for dtype in (np.float32, np.float64):
            host = lib._crba_host(x, dtype)
            rc, got = _device_run(lib, x, dtype)
            assert rc == 0
            assert not np.isnan(got).any(), "every output element must be written"
            assert np.array_equal(got, host)


def test_emulated_python_device_binding(emu):
    lib = emu("hyq")
    n = lib.n
    x = np.ascontiguousarray(states(n, 9, 2, 3 * n), dtype=np.float32)
    out = np.full((9, n * n), np.nan, dtype=np.float32)
    lib.crba_device(x.ctypes.data, 9, out.ctypes.data, stride=3 * n)
    assert np.array_equal(out, lib.crba_host(x))
    out2 = np.full((9, n * n), np.nan, dtype=np.float32)
    lib.crba_device(x.ctypes.data, 9, out2.ctypes.data)  # (default stride 3n: q_qd_u rows, as direct_minv_device)
    assert np.array_equal(out2, out)


def test_emulated_launch_dims_grid_stride(emu):
    lib = emu("iiwa14")
    n = lib.n
    x = states(n, 50, 4, n)
    ref = lib.crba_host(x)
    lib.set_launch_dims(blocks=2, threads=32)  # (few blocks: every lane group walks the batch)
    try:
        rc, got = _device_run(lib, x)
    finally:
        lib.set_launch_dims(0, 0)
    assert rc == 0 and np.array_equal(got, ref)


def test_emulated_boundary_cases(emu):
    lib = emu("hyq")
    L, H, n = lib.lib, lib.handle, lib.n
    q = np.zeros((4, 3 * n), dtype=np.float32)
    out = np.zeros((4, n * n), dtype=np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    NULL = ctypes.c_void_p(None)
    f = L.grid_crba_device
    assert f(H, NULL, n, 4, P(out), NULL) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n, 4, NULL, NULL) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n - 1, 4, P(out), NULL) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n, -1, P(out), NULL) == HIP_ERROR_INVALID_VALUE
    assert f(NULL, P(q), n, 4, P(out), NULL) == HIP_ERROR_INVALID_VALUE
    assert f(H, NULL, n, 0, NULL, NULL) == 0  # (an empty batch touches nothing)
    f = L.grid_crba_host
    assert f(H, NULL, n, 4, P(out)) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n, 4, NULL) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n - 1, 4, P(out)) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), 3 * n + 1, 4, P(out)) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n, -3, P(out)) == HIP_ERROR_INVALID_VALUE
    assert f(H, P(q), n, lib.max_timesteps + 1, P(out)) == HIP_ERROR_INVALID_VALUE
    assert f(NULL, P(q), n, 4, P(out)) == HIP_ERROR_INVALID_VALUE
    assert f(H, NULL, n, 0, NULL) == 0
    with pytest.raises(ValueError):
        lib.crba_host(np.zeros((4, n + 1), dtype=np.float32))
    # the handle still works after the rejected calls, and a longer call after a shorter one grows the staging
    assert lib.crba_host(q[:1]).shape == (1, n * n)
    assert np.array_equal(lib.crba_host(q)[0], lib.crba_host(q[:1])[0])


# ---------------------------------------------------------------------------------------------------- emitted surface
def test_emitted_surface(tmp_path):
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        src = GRiDCodeGenerator(RobotModel.from_fixture("iiwa14")).gen_all_code()  # (an 8-lane robot: its library has a nested `wide` namespace)
    finally:
        os.chdir(cwd)
    assert "namespace wide {" in src
    assert "void crba_inner_tip(" in src  # (a tip-frame robot: the inner of its formulation)
    for sfx in ("_device", "_kernel", "_kernel_single_timing", "", "_single_timing", "_compute_only"):
        assert ("void crba%s(" % sfx) in src, "crba" + sfx
    for k in ("LDS_PER_SOLVE", "OUT_PER_SOLVE", "SUGGESTED_THREADS", "DYNAMIC_SHARED_MEM_COUNT"):
        assert "const int CRBA_%s = " % k in src
    assert "const int CRBA_SHARED_MEM_COUNT = " in src  # (the reference's name)
    init = src[src.index("gridData<T> *init_gridData(int NUM_TIMESTEPS){"):]
    init = init[:init.index("return hd_data;")]
    assert "hd_data->d_M = nullptr;" in init and "hd_data->h_M = nullptr;" in init
    assert "grid_ee_release(&hd_data->d_M, &hd_data->h_M);" in src[src.index("void close_grid("):]
    assert src.index("grid_ee_reserve(T **d_buf") < src.index("grid_ee_reserve<T>(&hd_data->d_M")
    assert src.count("void crba_kernel(") == 1  # (the nested `wide` library does not repeat it)
    crba = src[src.index("// crba: joint-space inertia matrix"):]
    assert "__syncthreads" not in crba
    assert "Single Call CRBA" in crba
    for name in ("gen_crba", "gen_crba_inner", "gen_crba_inner_temp_mem_size", "gen_crba_inner_function_call", "gen_crba_device",
                 "gen_crba_device_temp_mem_size", "gen_crba_kernel", "gen_crba_host", "test_crba"):
        assert hasattr(GRiDCodeGenerator, name)


@pytest.mark.parametrize("name", FIXTURES)
def test_crba_constants_leave_the_existing_slices_alone(name):
    gen = GRiDCodeGenerator(RobotModel.from_fixture(name))
    lds = gen.gen_lds_layout()
    K = lds["KERNELS"]["CRBA"]
    n = gen.model.n
    assert K["OUT"] >= n * n
    if gen.branch_components:  # direct_minv's compact slice
        assert K["compact"] and (K["LDS"], K["SP"], K["MINV"]) == tuple(lds["KERNELS"]["MINV"][k] for k in ("LDS", "SP", "MINV"))
    else:  # a prefix of the general slice
        assert not K["compact"] and K["MINV"] + n * gen.minv_ld <= K["LDS"] <= lds["TOTAL"]
    assert set(lds["KERNELS"]) == {"ID", "ID_DU", "MINV", "FD", "ABA", "CRBA"}
