#!/usr/bin/env python
"""Timing of WaltonManolopoulosPropagator.norm() beyond 16 non-zero width modes (wm_pair_sum_wide_kernel).

    python tools/wm_norm_timing.py [--cases 24x24 51x45 60x60 80x72] [--n 1000 10000] [--profile]

Each case is an anharmonic AS model of D modes with a dense rotated width matrix of rank d' (D x d' in --cases).  One JSON
line per (case, n): norm() wall time from HIP events (the per-step export is cached by a first call, so the time is the
pair sum and its reduction), the FP64 flop model of the pair sum and its fraction of the measured 59 TFLOP/s FP64 VALU
rate (profiles/r4_bench_full_line.json).  --profile also runs each case in a child process under
rocprofv3 --kernel-trace --stats and adds the pair-sum kernel's own duration.

Flop model per ordered pair: complex LU of the d' x d' matrix 4/3 d'^3 real FMA, C_j dQ 2 D^2, U^T (.) 2 d' D; two flops
per FMA."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALU_TFS = 59.0


def make(D, dp, n, seed=3):
    from semiclassical_amd import propagators as PR
    rng = np.random.default_rng(seed)
    omega = np.sort(rng.uniform(600, 2500, D)) / 219474.63
    S = rng.uniform(0.05, 0.3, D) * rng.choice([-1, 1], D)
    q0 = torch.from_numpy(np.sqrt(2 * abs(S) / omega) * np.sign(S))
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    w = omega * rng.uniform(0.7, 1.4, D)
    w[dp:] = 0.0
    G = Q @ np.diag(w) @ Q.T
    G = torch.from_numpy(0.5 * (G + G.T))
    prop = PR.WaltonManolopoulosPropagator(G, G, 60.0, 60.0, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    assert prop._wm_host.dprime == dp
    return prop


def flops_per_pair(D, dp):
    return 2.0 * (4.0 / 3.0 * dp ** 3 + 2.0 * D * D + 2.0 * dp * D)


def measure(D, dp, n, reps):
    prop = make(D, dp, n)
    value = prop.norm()                         # exports the step's C_QQ, d once (cached for the timed calls)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        prop.norm()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    fl = flops_per_pair(D, dp) * float(n) * float(n)
    return {"D": D, "dprime": dp, "n": n, "reps": reps, "norm": value, "norm_ms": ms, "flops_model": fl,
            "fp64_frac_of_59_TFLOPs_wall": fl / (ms * 1e-3) / (VALU_TFS * 1e12)}


def kernel_ms(D, dp, n, reps):
    """the pair-sum kernel's mean duration from a rocprofv3 kernel trace of this script in a child process (top_kernels
    view of the rocpd database, durations in us, as tools/kernel_stats.py reads it)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--cases", f"{D}x{dp}", "--n", str(n), "--reps", str(reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=1200)
        db = glob.glob(os.path.join(tmp, "**", "*_results.db"), recursive=True)
        if not db:
            return None
        con = sqlite3.connect(db[0])
        cols = [r[1] for r in con.execute("pragma table_info(top_kernels)")]
        pick = lambda *names: next(cols.index(c) for c in names if c in cols)
        name_i, calls_i, total_i = cols.index("name"), pick("total_calls", "calls"), pick("total_duration", "total_duration (nsec)")
        rows = [r for r in con.execute("select * from top_kernels") if "wm_pair_sum" in r[name_i]]
        con.close()
    if not rows:
        return None
    calls = sum(int(r[calls_i]) for r in rows)
    total_us = sum(float(r[total_i]) for r in rows)
    return {"kernel": rows[0][name_i], "kernel_calls": calls, "kernel_ms": total_us / calls * 1e-3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["24x24", "51x45", "60x60", "80x72"])
    ap.add_argument("--n", type=int, nargs="*", default=[1000, 10000])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    for case in a.cases:
        D, dp = (int(v) for v in case.split("x"))
        for n in a.n:
            rec = measure(D, dp, n, a.reps)
            torch.cuda.empty_cache()
            if a.profile:
                k = kernel_ms(D, dp, n, a.reps)
                if k:
                    rec.update(k)
                    rec["fp64_frac_of_59_TFLOPs_kernel"] = rec["flops_model"] / (k["kernel_ms"] * 1e-3) / (VALU_TFS * 1e12)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
