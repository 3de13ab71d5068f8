#!/usr/bin/env python3
"""Records what a build returns for the launch shapes of tests/shell_cases.py (needs a GPU): inputs and the records of every case in one .npz.
tests/golden/kernel_shell/parent_<robot>.npz (a directory of their own: tests/test_crba.py takes every .npz directly under tests/golden for a robot's oracle vectors) were written by this tool from the build of the commit before include/grid_kernel_shell.h existed; the
kernel shell must keep reproducing them bit for bit (tests/test_gpu_kernel_shell.py).
usage: python tools/make_shell_golden.py <out-dir> <robot> [<robot> ...] [--build-dir <dir>]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gridcodegenerator_amd.runtime import load  # noqa: E402
from shell_cases import CASES, inputs, run_case  # noqa: E402


def main():
    args = sys.argv[1:]
    build_dir = None
    if "--build-dir" in args:
        i = args.index("--build-dir")
        build_dir = args[i + 1]
        args = args[:i] + args[i + 2:]
    out_dir, robots = args[0], args[1:]
    os.makedirs(out_dir, exist_ok=True)
    for name in robots:
        lib = load(name, max_timesteps=256, build_dir=build_dir)
        x = inputs(lib.n)
        data = {"x": x}
        for case in CASES:
            rec, guard = run_case(torch, lib, x, case)
            assert np.isfinite(rec).all() and np.isnan(guard).all(), (name, case)
            data[case] = rec
        lib.close()
        path = os.path.join(out_dir, "parent_%s.npz" % name)
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
