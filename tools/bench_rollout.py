#!/usr/bin/env python3
"""Fused rollout against the stepwise way of doing the same work, in one process on the same inputs:
  fused_traj / fused_xT  one rollout_device launch (with / without the per-step state store)
  stepwise               T launches of aba_device on one stream with a torch in-place update in between (state device-resident, no host sync inside)
  stepwise_graph         the same T steps captured once in a torch.cuda.graph and replayed (skipped with the reason if capture or replay fails)
The variants alternate inside every repetition; device events; min and median over the repetitions; us per step per batch.
usage: python tools/bench_rollout.py <robot> <batch> [steps=64] [reps=20] [--no-graph]"""
import json, sys
sys.path.insert(0, ".")
import numpy as np, torch
from gridcodegenerator_amd import RobotModel
from gridcodegenerator_amd.runtime import load
args = [a for a in sys.argv[1:] if not a.startswith("--")]
name, N = args[0], int(args[1])
T = int(args[2]) if len(args) > 2 else 64
reps = int(args[3]) if len(args) > 3 else 20
DT = 1e-3
n = RobotModel.from_fixture(name).n
lib = load(name, max_timesteps=N)
rng = np.random.default_rng(0)
x0 = rng.uniform(-1, 1, (N, 2 * n)).astype(np.float32)
u = rng.uniform(-5, 5, (T, N, n)).astype(np.float32)
stream = torch.cuda.Stream()
st = stream.cuda_stream
with torch.cuda.stream(stream):
    d_x0 = torch.from_numpy(np.hstack([x0, u[0]])).cuda()  # (N, 3n)
    d_u = torch.from_numpy(u).cuda()
    d_traj = torch.empty((T + 1, N, 2 * n), dtype=torch.float32, device="cuda")
    d_xT = torch.empty((N, 2 * n), dtype=torch.float32, device="cuda")
    d_x = d_x0.clone()
    d_qdd = torch.empty((N, n), dtype=torch.float32, device="cuda")


def fused_traj():
    lib.rollout_device(d_x0, d_u, N, T, DT, d_traj=d_traj, stride_x0=3 * n, stream=st)


def fused_xT():
    lib.rollout_device(d_x0, d_u, N, T, DT, d_xT=d_xT, stride_x0=3 * n, stream=st)


def steps():
    for t in range(T):
        d_x[:, 2 * n:].copy_(d_u[t])
        lib.aba_device(d_x, N, d_qdd, stream=st)
        d_x[:, n:2 * n].add_(d_qdd, alpha=DT)
        d_x[:, :n].add_(d_x[:, n:2 * n], alpha=DT)


def stepwise():
    d_x.copy_(d_x0)
    steps()


cases = [("fused_traj", fused_traj), ("fused_xT", fused_xT), ("stepwise", stepwise)]
graph_note = None
if "--no-graph" in sys.argv:
    graph_note = "not attempted (--no-graph)"
else:
    try:
        with torch.cuda.stream(stream):
            stepwise()
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                stepwise()
            g.replay()
            stream.synchronize()
        cases.append(("stepwise_graph", g.replay))
    except Exception as e:  # (reported, not hidden: the row says why there is no number)
        graph_note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])
with torch.cuda.stream(stream):
    for _ in range(3):
        for _, fn in cases:
            fn()
    stream.synchronize()
    # same work, same result (to the fp32 bar: the kernel may contract the update to an FMA)
    fused_xT(); stepwise(); stream.synchronize()
    a, b = d_xT.double(), d_x[:, :2 * n].double()
    agree = float(((a - b).abs().amax(dim=1) / b.abs().amax(dim=1).clamp(min=1.0)).max())
    times = {nm: [] for nm, _ in cases}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    inner = max(1, int(4096 * 64 / (N * T)) * 2)  # (a timed window is at least a few milliseconds)
    for rep in range(reps):
        for nm, fn in cases:
            e0.record(stream)
            for _ in range(inner):
                fn()
            e1.record(stream)
            stream.synchronize()
            times[nm].append(1e3 * e0.elapsed_time(e1) / inner)
for nm, _ in cases:
    v = np.array(times[nm])
    print(json.dumps({"robot": name, "batch": N, "steps": T, "variant": nm, "us_per_rollout_min": round(float(v.min()), 1), "us_per_rollout_median": round(float(np.median(v)), 1),
                      "us_per_step_min": round(float(v.min()) / T, 3), "us_per_step_median": round(float(np.median(v)) / T, 3), "reps": reps, "launches_per_rep": inner,
                      "fused_vs_stepwise_max_rel_diff": agree}))
if graph_note:
    print(json.dumps({"robot": name, "batch": N, "steps": T, "variant": "stepwise_graph", "skipped": graph_note}))
lib.close()
