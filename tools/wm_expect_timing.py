#!/usr/bin/env python
"""Timing of WaltonManolopoulosPropagator.wm_expectation() against norm() on the same state.

    python tools/wm_expect_timing.py [--cases 24x24 5x5] [--n 2000] [--rounds 3] [--out profiles/wm_expect_timing.jsonl]

Each case is the anharmonic AS model of tools/wm_norm_timing.py: D modes, a dense rotated width matrix of rank d' (D x d' in
--cases); 24x24 is the shape of the wm_as24 fixture, 5x5 that of wm_as5_chi002.  HIP events around whole calls (the fold of the
operators, the columns, every launch of the pair kernel and the copy of the result; the per-step export is cached by a first
call), --rounds rounds of one call each, the median kept.  One JSON line per (case, call):
    norm            norm()
    constant        wm_expectation(c=[1])                               1 column
    x_p_4           wm_expectation(x=4 directions, p=4 directions)      8 operators, 8 columns
    xx_full         wm_expectation(xx=[one matrix of rank d'])          1 + d' columns
with the time in ms and as a multiple of norm()."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(call, rounds):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    from wm_norm_timing import make
    from semiclassical_amd._lib import lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["24x24", "5x5"])
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wm_expect_timing.jsonl"))
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    lines = []
    for case in a.cases:
        D, dp = (int(v) for v in case.split("x"))
        prop = make(D, dp, a.n)
        U = prop._wm_host.U.numpy()
        rng = np.random.default_rng(7)
        dirs = (U @ rng.standard_normal((dp, 4))).T
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        zeros = np.zeros_like(dirs)
        V = U @ np.linalg.qr(rng.standard_normal((dp, dp)))[0]
        K = (V * rng.uniform(0.5, 2.0, dp)) @ V.T
        K = 0.5 * (K + K.T)
        calls = [("norm", prop.norm),
                 ("constant", lambda: prop.wm_expectation(c=np.ones(1))),
                 ("x_p_4", lambda: prop.wm_expectation(x=np.concatenate((dirs, zeros)), p=np.concatenate((zeros, dirs)))),
                 ("xx_full", lambda: prop.wm_expectation(xx=K[None]))]
        base = None
        for name, call in calls:
            ms = timed(call, a.rounds)
            med = float(np.median(ms))
            base = med if name == "norm" else base
            rec = {"D": D, "dprime": dp, "n": a.n, "call": name, "rounds_ms": ms, "ms": med, "times_norm": med / base,
                   "columns_per_launch": int(lib.sc_wm_pair_expect_capacity(D, dp))}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        del prop
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
