#!/usr/bin/env python3
"""Parity of the fused rollout on the GPU against the stepwise fp64 oracle rollout (tests/rollout_reference.py): every solve, every step.
Per-solve error max|got - ref| / max(1, max|ref|); q0, qd0 ~ U(-1, 1), u ~ U(-5, 5), dt = 1e-3, 64 steps.  One JSON line per robot and batch.
usage: python tests/tools/parity_sweep_rollout.py [robot[:batch] ...]"""
import json, sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
from gridcodegenerator_amd.runtime import load
from rollout_reference import FIXTURES, inputs, oracle_rollout, per_solve_err

T, DT = 64, 1e-3
for spec in sys.argv[1:] or [r + ":1000" for r in FIXTURES]:
    name, N = spec.split(":")[0], int(spec.split(":")[1]) if ":" in spec else 1000
    lib = load(name, max_timesteps=N)
    x0, u = inputs(lib.n, N, T, 31)
    ref = oracle_rollout(name, x0, u, DT)
    e32 = per_solve_err(lib.rollout_host(x0, u, DT), ref)
    e64 = per_solve_err(lib.rollout_host_f64(x0.astype(np.float64), u.astype(np.float64), DT), ref)
    print(json.dumps({"robot": name, "batch": N, "steps": T, "dt": DT, "fp32_max": float(e32.max()), "fp32_p999": float(np.quantile(e32, 0.999)), "fp32_median": float(np.median(e32)),
                      "fp32_worst_solve": int(e32.argmax()), "fp64_max": float(e64.max()), "solves_compared": int(e32.size), "solves_skipped": 0}), flush=True)
    lib.close()
