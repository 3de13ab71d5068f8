#!/usr/bin/env python3
"""Linearised rollout against the stepwise way of getting the same records, in one process on the same inputs (device-resident, HIP events):
  fused            one rollout_linearized_device launch, all outputs (traj, fx, fu)
  fused_fx_only    the same launch writing fx alone (no M^-1 work where that is separate, no fu / traj traffic)
  stepwise         per step: forward_dynamics_gradient_device + direct_minv_device + aba_device on one stream and the torch in-place update (no host sync inside)
  stepwise_graph   the same T steps captured once in a torch.cuda.graph and replayed (skipped with the reason if capture or replay fails)
The baseline uses entry points that exist without rollout_linearized only.  The variants alternate inside every repetition; min and median over the repetitions;
us per step per batch; achieved output bandwidth of `fused` (3n^2 + 2n values per step and solve over kernel time).
usage: python tools/bench_rollout_linearized.py <robot> <batch> [steps=64] [reps=20] [--no-graph]"""
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
    E = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    d_x0 = torch.from_numpy(np.hstack([x0, u[0]])).cuda()  # (N, 3n)
    d_u = torch.from_numpy(u).cuda()
    d_traj, d_fx, d_fu = E(T + 1, N, 2 * n), E(T, N, 2 * n * n), E(T, N, n * n)
    s_traj, s_fx, s_fu = E(T + 1, N, 2 * n), E(T, N, 2 * n * n), E(T, N, n * n)  # the stepwise path writes the same records
    d_x = d_x0.clone()
    d_qdd = E(N, n)


def fused():
    lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_traj=d_traj, d_fx=d_fx, d_fu=d_fu, stride_x0=3 * n, stream=st)


def fused_fx_only():
    lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_fx=d_fx, stride_x0=3 * n, stream=st)


def stepwise():
    d_x.copy_(d_x0)
    s_traj[0].copy_(d_x[:, :2 * n])
    for t in range(T):
        d_x[:, 2 * n:].copy_(d_u[t])
        lib.forward_dynamics_gradient_device(d_x, N, s_fx[t], stream=st)
        lib.direct_minv_device(d_x, N, s_fu[t], stream=st)
        lib.aba_device(d_x, N, d_qdd, stream=st)
        d_x[:, n:2 * n].add_(d_qdd, alpha=DT)
        d_x[:, :n].add_(d_x[:, n:2 * n], alpha=DT)
        s_traj[t + 1].copy_(d_x[:, :2 * n])


cases = [("fused", fused), ("fused_fx_only", fused_fx_only), ("stepwise", stepwise)]
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
    for _ in range(3):  # warm-up of every shape
        for _, fn in cases:
            fn()
    stream.synchronize()
    # same work, same records (to the fp32 bar)
    fused(); stepwise(); stream.synchronize()
    rel = lambda a, b: float(((a.double() - b.double()).abs().amax(dim=-1) / b.double().abs().amax(dim=-1).clamp(min=1e-30)).max())
    agree = {"traj": float(((d_traj.double() - s_traj.double()).abs().amax(dim=(0, 2)) / s_traj.double().abs().amax(dim=(0, 2)).clamp(min=1.0)).max()), "fx": rel(d_fx, s_fx)}
    times = {nm: [] for nm, _ in cases}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    inner = max(1, int(4096 * 64 / (N * T)))
    for rep in range(reps):
        for nm, fn in cases:
            e0.record(stream)
            for _ in range(inner):
                fn()
            e1.record(stream)
            stream.synchronize()
            times[nm].append(1e3 * e0.elapsed_time(e1) / inner)
out_bytes = 4.0 * (3 * n * n + 2 * n) * N * T
for nm, _ in cases:
    v = np.array(times[nm])
    row = {"robot": name, "batch": N, "steps": T, "variant": nm, "us_per_rollout_min": round(float(v.min()), 1), "us_per_rollout_median": round(float(np.median(v)), 1),
           "us_per_rollout_max": round(float(v.max()), 1), "us_per_step_min": round(float(v.min()) / T, 3), "us_per_step_median": round(float(np.median(v)) / T, 3),
           "reps": reps, "launches_per_rep": inner, "fused_vs_stepwise_max_rel_diff": agree}
    if nm == "fused":
        row["output_GBps_median"] = round(out_bytes / (float(np.median(v)) * 1e-6) / 1e9, 1)
    print(json.dumps(row))
if graph_note:
    print(json.dumps({"robot": name, "batch": N, "steps": T, "variant": "stepwise_graph", "skipped": graph_note}))
lib.close()
