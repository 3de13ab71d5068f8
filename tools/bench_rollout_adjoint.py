#!/usr/bin/env python3
"""Rollout adjoint against the way of getting the same gradients without it, in one process on the same inputs (device-resident, HIP events):
  fused             one rollout_adjoint_device launch writing grad_x0 + grad_u from traj, u and gx
  fused_x0_only     the same launch writing grad_x0 alone (no M^-1 work where that is separate)
  baseline          rollout_linearized_device writing fx + fu (3n^2 values per solve and step), then the reverse recurrence in torch (discrete_jacobians is
                    not materialised: the collapsed step as two batched mat-vecs per step on views of fx and fu)
  baseline_graph    the same, captured once in a torch.cuda.graph and replayed (skipped with the reason if capture or replay fails)
  linearized_fx     for context: rollout_linearized_device writing fx alone on the same batch (a reverse step should cost about one such step plus the mat-vecs)
  torch_fwd_bwd     rollout_torch forward (rollout) + backward (rollout_adjoint) through autograd, both gradients
The variants alternate inside every repetition; min, median and max over the repetitions; us per step per batch.
usage: python tools/bench_rollout_adjoint.py <robot> <batch> [steps=64] [reps=20] [--no-graph]"""
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
g = rng.uniform(-1, 1, (T + 1, N, 2 * n)).astype(np.float32)
stream = torch.cuda.Stream()
st = stream.cuda_stream
with torch.cuda.stream(stream):
    E = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    d_x0, d_u, d_g = torch.from_numpy(x0).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(g).cuda()
    d_traj, d_fx, d_fu = E(T + 1, N, 2 * n), E(T, N, 2 * n * n), E(T, N, n * n)
    d_gx0, d_gu = E(N, 2 * n), E(T, N, n)
    b_gx0, b_gu = E(N, 2 * n), E(T, N, n)
    lib.rollout_device(d_x0, d_u, N, T, DT, d_traj=d_traj, stream=st)
    t_x0, t_u = d_x0.clone().requires_grad_(True), d_u.clone().requires_grad_(True)


def fused():
    lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_g, d_grad_x0=d_gx0, d_grad_u=d_gu, stream=st)


def fused_x0_only():
    lib.rollout_adjoint_device(d_traj, d_u, N, T, DT, d_gx=d_g, d_grad_x0=d_gx0, stream=st)


def linearized_fx():
    lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_fx=d_fx, stream=st)


def baseline():
    lib.rollout_linearized_device(d_x0, d_u, N, T, DT, d_fx=d_fx, d_fu=d_fu, stream=st)
    F = d_fx.view(T, N, 2 * n, n)  # [t, k, col, row]: F[t, k, c] is column c of [Fq | Fv]
    M = d_fu.view(T, N, n, n)
    lq, lv = d_g[T, :, :n], d_g[T, :, n:]
    for t in range(T - 1, -1, -1):
        w = lv + DT * lq
        torch.matmul(M[t], w.unsqueeze(-1), out=b_gu[t].unsqueeze(-1))  # (symmetric M^-1)
        Fw = torch.matmul(F[t], w.unsqueeze(-1)).squeeze(-1)  # (N, 2n): [Fq^T w | Fv^T w]
        lq = d_g[t, :, :n] + lq + DT * Fw[:, :n]
        lv = d_g[t, :, n:] + w + DT * Fw[:, n:]
    b_gu.mul_(DT)
    b_gx0[:, :n].copy_(lq)
    b_gx0[:, n:].copy_(lv)


def torch_fwd_bwd():
    t_x0.grad, t_u.grad = None, None
    traj = lib.rollout_torch(t_x0, t_u, DT)
    traj.backward(d_g)


cases = [("fused", fused), ("fused_x0_only", fused_x0_only), ("baseline", baseline), ("linearized_fx", linearized_fx), ("torch_fwd_bwd", torch_fwd_bwd)]
graph_note = None
if "--no-graph" in sys.argv:
    graph_note = "not attempted (--no-graph)"
else:
    try:
        with torch.cuda.stream(stream):
            baseline()
            stream.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=stream):
                baseline()
            gr.replay()
            stream.synchronize()
        cases.insert(3, ("baseline_graph", gr.replay))
    except Exception as e:  # (reported, not hidden: the row says why there is no number)
        graph_note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])
with torch.cuda.stream(stream):
    for _ in range(3):  # warm-up of every shape
        for _, fn in cases:
            fn()
    stream.synchronize()
    # same work, same records (to the fp32 bar): per solve max|d| / max|ref|
    fused(); baseline(); stream.synchronize()
    rel = lambda a, b, dims: float(((a.double() - b.double()).abs().amax(dim=dims) / b.double().abs().amax(dim=dims).clamp(min=1e-30)).max())
    agree = {"grad_x0": rel(d_gx0, b_gx0, (1,)), "grad_u": rel(d_gu, b_gu, (0, 2))}
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
for nm, _ in cases:
    v = np.array(times[nm])
    row = {"robot": name, "batch": N, "steps": T, "variant": nm, "us_per_pass_min": round(float(v.min()), 1), "us_per_pass_median": round(float(np.median(v)), 1),
           "us_per_pass_max": round(float(v.max()), 1), "us_per_step_min": round(float(v.min()) / T, 3), "us_per_step_median": round(float(np.median(v)) / T, 3),
           "us_per_step_max": round(float(v.max()) / T, 3), "reps": reps, "launches_per_rep": inner, "fused_vs_baseline_max_rel_diff": agree}
    print(json.dumps(row))
if graph_note:
    print(json.dumps({"robot": name, "batch": N, "steps": T, "variant": "baseline_graph", "skipped": graph_note}))
lib.close()
