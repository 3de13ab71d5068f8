"""GPU tests of the hand-written kernel shell (include/grid_kernel_shell.h) behind forward_dynamics_gradient_kernel of the tip-frame robots: input staging
at the head, model constants into registers, wave-cooperative copy-out at the tail.  The shell changes no arithmetic, so

  * every launch shape of tests/shell_cases.py reproduces, bit for bit, what the build of the commit before the shell returned on an MI355X
    (tests/golden/kernel_shell/parent_<robot>.npz, recorded by tools/make_shell_golden.py) - 7-joint arm (8-lane groups, interleaved) and quadruped
    (forest, 16-lane groups);
  * every entry of the N records is written, nothing behind them (or in front of an offset base) is touched;
  * the same records agree with the fp64 oracle to the bound of tests/test_gpu_parity.py - what keeps the test meaningful once the fixture's
    parent is long gone.
"""
import numpy as np
import pytest
from shell_cases import CASES, inputs, run_case

from gridcodegenerator_amd import RobotModel
from gridcodegenerator_amd.runtime import GridLibrary, build_library

pytestmark = pytest.mark.gpu
TOL = 1e-4  # per solve max|delta| <= TOL * max|reference| (tests/test_gpu_parity.py)
ROBOTS = ["iiwa14", "hyq"]


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
            cache[name] = GridLibrary(build_library(name), device=0, max_timesteps=256)  # raises when the HIP .so is missing
        return cache[name]

    yield get
    for lib in cache.values():
        lib.close()


@pytest.fixture(scope="module")
def oracle_records():
    """fp64 oracle records of the N_MAX states of shell_cases.inputs, computed once per robot; every case compares its first N rows."""
    cache = {}

    def get(name):
        if name not in cache:
            from oracle.rbd_oracle import Oracle

            robot = RobotModel.from_fixture(name)
            ref, _ = Oracle(robot).fd_grad_batch(inputs(robot.n).astype(np.float64))
            ref.setflags(write=False)
            cache[name] = ref
        return cache[name]

    return get


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ROBOTS)
def test_shell_reproduces_the_parent_build_bit_for_bit(name, case, torch_cuda, libs, golden, oracle_records):
    g = golden("kernel_shell/parent_" + name)
    lib = libs(name)
    x = inputs(lib.n)
    assert np.array_equal(x, g["x"])  # (the fixture's inputs are the seeded ones)
    rec, guard = run_case(torch_cuda, lib, x, case)
    N = CASES[case][0]
    assert not np.isnan(rec).any(), "an entry of the N records was not written"
    assert np.isnan(guard).all(), "the kernel wrote outside the N records"
    assert np.array_equal(rec, g[case]), "not the parent build's bits"
    ref = oracle_records(name)[:N]
    err = (np.abs(rec.astype(np.float64) - ref).max(axis=1) / np.abs(ref).max(axis=1)).max()
    assert err <= TOL, err
