#!/usr/bin/env python3
"""Closed-loop rollout against the stepwise way of doing the same work, in one process per row on the same inputs (T = 64, device-resident, limits on):
  fused            one rollout_feedback_device launch: dense K (T, N, 2n^2), limits, traj + u_out written
  fused_xT         the same without the per-step stores (xT only)
  fused_shared_K   one gain for all solves and steps, traj + u_out
  rollout          the open-loop rollout_device on the same shapes (traj): the price of the law is fused / rollout
  stepwise         what the library offered before: per step a torch batched mat-vec, clamp, aba_device and the in-place update on one stream, no host sync
  stepwise_graph   the same T steps captured once in a torch.cuda.graph (default queue settings) and replayed (skipped with the reason if capture or replay fails)
The variants alternate inside every repetition; device events; every shape is warmed first; min (median) [max] over the repetitions.
usage: python tools/bench_rollout_feedback.py                      all rows, one child process each, results appended to profiles/r09_rollout_feedback.jsonl
       python tools/bench_rollout_feedback.py <robot> <batch> [steps=64] [reps=20] [--no-graph]      one row, JSON lines on stdout"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ROWS = [("iiwa14", 16384), ("iiwa14", 2048), ("hyq", 4096), ("atlas", 2048), ("mixed5", 16384)]


def all_rows():
    out_path = os.path.join(REPO, "profiles", "r09_rollout_feedback.jsonl")
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    with open(out_path, "w") as out:
        for name, N in ROWS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(N)] + flags, capture_output=True, text=True, timeout=900)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:  # (a failed row ends the visit: nothing more is started on the card)
                sys.stderr.write(r.stderr[-4000:])
                sys.exit(r.returncode)
            out.write(r.stdout)
            out.flush()


def one_row(args):
    import numpy as np
    import torch

    from gridcodegenerator_amd import RobotModel
    from gridcodegenerator_amd.runtime import load

    name, N = args[0], int(args[1])
    T = int(args[2]) if len(args) > 2 else 64
    reps = int(args[3]) if len(args) > 3 else 20
    DT, LIM = 1e-3, 4.0
    n = RobotModel.from_fixture(name).n
    lib = load(name, max_timesteps=N)
    rng = np.random.default_rng(0)
    x0 = rng.uniform(-1, 1, (N, 2 * n)).astype(np.float32)
    u = rng.uniform(-5, 5, (T, N, n)).astype(np.float32)
    x_ref = rng.uniform(-1, 1, (T, N, 2 * n)).astype(np.float32)
    Kmat = (-np.hstack([np.eye(n), 0.02 * np.eye(n)]) + rng.uniform(-0.02, 0.02, (T, N, n, 2 * n))).astype(np.float32)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    with torch.cuda.stream(stream):
        d_x0 = torch.from_numpy(np.hstack([x0, u[0]])).cuda()  # (N, 3n)
        d_u, d_xr = torch.from_numpy(u).cuda(), torch.from_numpy(x_ref).cuda()
        d_Kmat = torch.from_numpy(Kmat).cuda()                                      # (T, N, n, 2n): what torch.bmm reads
        d_K = d_Kmat.transpose(2, 3).contiguous().reshape(T, N, 2 * n * n)          # records [c*n + j]: what the kernel reads
        d_K0 = d_K[0, 0].contiguous()
        d_lo, d_hi = torch.full((n,), -LIM, device="cuda"), torch.full((n,), LIM, device="cuda")
        d_traj = torch.empty((T + 1, N, 2 * n), dtype=torch.float32, device="cuda")
        d_uo = torch.empty((T, N, n), dtype=torch.float32, device="cuda")
        d_xT = torch.empty((N, 2 * n), dtype=torch.float32, device="cuda")
        d_x = d_x0.clone()
        d_qdd = torch.empty((N, n), dtype=torch.float32, device="cuda")
        d_dx = torch.empty((N, 2 * n, 1), dtype=torch.float32, device="cuda")
        d_v = torch.empty((N, n, 1), dtype=torch.float32, device="cuda")
    lim = dict(d_u_min=d_lo, d_u_max=d_hi, stride_x0=3 * n, stream=st)

    def fused():
        lib.rollout_feedback_device(d_x0, d_u, d_K, d_xr, N, T, DT, d_traj=d_traj, d_u_out=d_uo, **lim)

    def fused_xT():
        lib.rollout_feedback_device(d_x0, d_u, d_K, d_xr, N, T, DT, d_xT=d_xT, **lim)

    def fused_shared_K():
        lib.rollout_feedback_device(d_x0, d_u, d_K0, d_xr, N, T, DT, d_traj=d_traj, d_u_out=d_uo, K_strides=(0, 0), **lim)

    def rollout():
        lib.rollout_device(d_x0, d_u, N, T, DT, d_traj=d_traj, stride_x0=3 * n, stream=st)

    def stepwise():
        d_x.copy_(d_x0)
        for t in range(T):
            torch.sub(d_x[:, :2 * n], d_xr[t], out=d_dx[:, :, 0])
            torch.bmm(d_Kmat[t], d_dx, out=d_v)
            torch.add(d_v[:, :, 0], d_u[t], out=d_x[:, 2 * n:])
            d_x[:, 2 * n:].clamp_(min=-LIM, max=LIM)
            lib.aba_device(d_x, N, d_qdd, stream=st)
            d_x[:, n:2 * n].add_(d_qdd, alpha=DT)
            d_x[:, :n].add_(d_x[:, n:2 * n], alpha=DT)

    cases = [("fused", fused), ("fused_xT", fused_xT), ("fused_shared_K", fused_shared_K), ("rollout", rollout), ("stepwise", stepwise)]
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
        # same work, same result (to the fp32 bar: other summation order in bmm, possible FMA contraction)
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
    v = {nm: np.array(times[nm]) for nm, _ in cases}
    base = [nm for nm in ("stepwise", "stepwise_graph") if nm in v]
    for nm, _ in cases:
        row = {"robot": name, "batch": N, "steps": T, "variant": nm, "us_per_rollout_min": round(float(v[nm].min()), 1), "us_per_rollout_median": round(float(np.median(v[nm])), 1),
               "us_per_rollout_max": round(float(v[nm].max()), 1), "us_per_step_median": round(float(np.median(v[nm])) / T, 3), "reps": reps, "launches_per_rep": inner}
        if nm == "fused":
            row["fused_vs_stepwise_max_rel_diff"] = agree
            row["law_price_vs_rollout_median"] = round(float(np.median(v["fused"]) / np.median(v["rollout"])), 3)
            for b_ in base:
                row["speedup_vs_%s_median" % b_] = round(float(np.median(v[b_]) / np.median(v["fused"])), 2)
            row["slowest_fused_beats_fastest_baseline"] = bool(all(v["fused"].max() < v[b_].min() for b_ in base))
        print(json.dumps(row))
    if graph_note:
        print(json.dumps({"robot": name, "batch": N, "steps": T, "variant": "stepwise_graph", "skipped": graph_note}))
    lib.close()


if __name__ == "__main__":
    positional = [a for a in sys.argv[1:] if not a.startswith("--")]
    if positional:
        one_row(positional)
    else:
        all_rows()
