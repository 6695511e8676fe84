#!/usr/bin/env python
"""Timing of WaltonManolopoulosPropagator.wm_operator_expectation() / wm_energy_expectation() against norm() and wm_expectation() on
the same state.

    python tools/wm_energy_timing.py [--cases 24x24 5x5] [--n 2000] [--rounds 3] [--out profiles/wm_energy_timing.jsonl]

The model and the method of tools/wm_expect_timing.py: the anharmonic AS model of tools/wm_norm_timing.py, HIP events around whole
calls (fold, columns, every launch, the copy of the result; the per-step export is cached by a first call), --rounds rounds of one
call each, the median kept.  One JSON line per (case, call):
    norm            norm()
    xx_full         wm_expectation(xx=[one matrix of rank d'])              1 + d' columns, fixed border vectors, sc_wm_pair_expect
    pp_full         wm_operator_expectation(pp=[one matrix of rank d'])     1 + d' columns, per-ket border vectors, sc_wm_pair_expect_cols
    morse_energy    wm_energy_expectation(MorsePotential, chi = 0.02)       1 + d' + 2 d' columns (73 at D = 24: one call)
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


def main():
    from wm_expect_timing import timed
    from wm_norm_timing import make
    from semiclassical_amd import potentials as P
    from semiclassical_amd._lib import lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["24x24", "5x5"])
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wm_energy_timing.jsonl"))
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    lines = []
    for case in a.cases:
        D, dp = (int(v) for v in case.split("x"))
        assert D == dp, "<H> needs widths of full rank"
        prop = make(D, dp, a.n)
        omega = np.sort(np.random.default_rng(3).uniform(600, 2500, D)) / 219474.63         # the frequencies make() draws first
        pot = P.MorsePotential(torch.from_numpy(omega), torch.full((D,), 0.02), torch.zeros(D))
        U = prop._wm_host.U.numpy()
        rng = np.random.default_rng(7)
        V = U @ np.linalg.qr(rng.standard_normal((dp, dp)))[0]
        K = (V * rng.uniform(0.5, 2.0, dp)) @ V.T
        K = 0.5 * (K + K.T)
        calls = [("norm", prop.norm),
                 ("xx_full", lambda: prop.wm_expectation(xx=K[None])),
                 ("pp_full", lambda: prop.wm_operator_expectation(pp=K[None])),
                 ("morse_energy", lambda: prop.wm_energy_expectation(pot))]
        columns = {"norm": 0, "xx_full": 1 + dp, "pp_full": 1 + dp, "morse_energy": 1 + 3 * dp}
        base = None
        for name, call in calls:
            ms = timed(call, a.rounds)
            med = float(np.median(ms))
            base = med if name == "norm" else base
            rec = {"D": D, "dprime": dp, "n": a.n, "call": name, "columns": columns[name], "rounds_ms": ms, "ms": med,
                   "times_norm": med / base, "columns_per_launch": int(lib.sc_wm_pair_expect_capacity(D, dp))}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        del prop
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
