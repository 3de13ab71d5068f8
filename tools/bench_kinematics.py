"""Timing of the end-effector kinematics kernels (end_effector_pose / _gradient / _gradient_hessian) through the C ABI, with HIP events.

    python tools/bench_kinematics.py --robot iiwa14 --batch 16384 [--kernels pose,gradient,hessian] [--reps 200] [--warmup 20] [--out FILE.jsonl]

One JSON line per kernel: us per launch, solves/s, algorithmic bytes (q read + record written) and their fraction of the 8 TB/s HBM peak, and -
measured in the same process on the same robot and batch - forward_dynamics_gradient_device as a yardstick.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gridcodegenerator_amd.runtime import GridLibrary, build_library  # noqa: E402

HBM_PEAK = 8.0e12


def time_launch(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="iiwa14")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--kernels", default="pose,gradient,hessian")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    lib = GridLibrary(build_library(a.robot), device=0, max_timesteps=16)
    n, E, N = lib.n, lib.num_end_effectors, a.batch
    s = torch.cuda.current_stream().cuda_stream
    q = torch.from_numpy(np.random.default_rng(0).uniform(-np.pi, np.pi, (N, n)).astype(np.float32)).cuda()
    x = torch.from_numpy(np.random.default_rng(1).uniform(-2, 2, (N, 3 * n)).astype(np.float32)).cuda()
    df = torch.empty((N, 2 * n * n), dtype=torch.float32, device="cuda")
    fdg = time_launch(torch, lambda: lib.forward_dynamics_gradient_device(x, N, df, stream=s), a.reps, a.warmup)
    lines = []
    for k in a.kernels.split(","):
        rec = {"pose": 6 * E, "gradient": 6 * E * n, "hessian": 6 * E * n * n}[k]
        out = torch.empty((N, rec), dtype=torch.float32, device="cuda")
        if k == "pose":
            fn = lambda: lib.end_effector_pose_device(q, N, out, stream=s)
        elif k == "gradient":
            fn = lambda: lib.end_effector_pose_gradient_device(q, N, out, stream=s)
        else:
            fn = lambda: lib.end_effector_pose_gradient_hessian_device(q, N, out, None, stream=s)  # (Hessian alone: d_deePos = NULL)
        us = time_launch(torch, fn, a.reps, a.warmup)
        nbytes = 4 * N * (n + rec)
        line = {"robot": a.robot, "batch": N, "kernel": "end_effector_" + k, "us_per_launch": round(us, 3), "solves_per_s": round(N / us * 1e6),
                "algorithmic_bytes": nbytes, "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
                "fd_grad_us_same_process": round(fdg, 3), "ratio_vs_fd_grad": round(us / fdg, 3), "device": torch.cuda.get_device_name(0)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    lib.close()


if __name__ == "__main__":
    main()
