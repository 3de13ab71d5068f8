"""CPU emulation of the hand-written kernel shell (include/grid_kernel_shell.h): the launch shapes of tests/shell_cases.py - the ones at which the input
staging and the wave-cooperative copy-out can go wrong - through the emulation build of the generated header, against the fp64 oracle (bound of
tests/test_generated_emulation.py).  Every entry of the N records is written and nothing around them.  Emulation bits need not equal the GPU's; the
GPU counterpart, tests/test_gpu_kernel_shell.py, pins those."""
import numpy as np
import pytest
from emu_harness import emu_library
from shell_cases import CASES, inputs, run_case

from gridcodegenerator_amd import RobotModel

TOL = 1e-4


@pytest.mark.parametrize("name,shell,cases", [("iiwa14", None, list(CASES)), ("hyq", None, list(CASES)),
                                              # the parts that are not shipped (tuning "shell") and the emitted shell, at a ragged and a grid-stride shape
                                              ("iiwa14", "inputs,qreg,consts,store,chain", ["n9", "n65_one_block"]), ("hyq", "inputs,qreg,consts,store,chain", ["n9", "n65_one_block"]),
                                              ("iiwa14", "inputs", ["n9"]), ("iiwa14", "", ["n9"])])
def test_emulated_shell_shapes_match_the_oracle(name, shell, cases):
    from oracle.rbd_oracle import Oracle

    robot = RobotModel.from_fixture(name)
    tuning = {"so_lanes": "off"}  # (first-order checks only: no second library instance to compile)
    if shell is not None:
        tuning["shell"] = shell
    lib = emu_library(name, max_timesteps=256, tuning=tuning)
    x = inputs(robot.n)
    ref, _ = Oracle(robot).fd_grad_batch(x.astype(np.float64))
    try:
        for case in cases:
            N = CASES[case][0]
            rec, guard = run_case(None, lib, x, case)
            assert not np.isnan(rec).any(), case
            assert np.isnan(guard).all(), case
            err = (np.abs(rec.astype(np.float64) - ref[:N]).max(axis=1) / np.abs(ref[:N]).max(axis=1)).max()
            assert err <= TOL, (case, err)
    finally:
        lib.close()
