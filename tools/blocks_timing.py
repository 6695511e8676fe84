#!/usr/bin/env python
"""Wall time of run() with and without error blocks (run(..., blocks=...)).

    python tools/blocks_timing.py [out.jsonl] [B]

Cases: the headline (separable D = 60, n = 1e5, 200 steps: two-step pairs), the whole-loop kernel (as5, n = 1e5) and WM as24.
Each configuration is warmed up once, then timed over three runs from fresh initial conditions; the median is reported together
with the three figures (their spread is what "equal to the parent commit" is judged by with blocks off)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases, engine_cases  # noqa: E402
from semiclassical_amd import propagators as PR  # noqa: E402

CASES = [("headline_as60", "hk_as60", 100000, 200), ("whole_loop_as5", "hk_as5_chi002", 100000, 200),
         ("wm_as24", "wm_as24", 10000, 50)]


def one(g, n, nt, nblocks):
    pot, dt = engine_cases.engine_potential(g), float(g["dt"])
    Gi, Gt = cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"])
    prop = (PR.WaltonManolopoulosPropagator(Gi, Gt, float(g["alpha"]), float(g["beta"])) if "alpha" in g
            else PR.HermanKlukPropagator(Gi, Gt))
    prop.initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), ntraj=n, seed=5)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    blocks = torch.zeros((nt, nblocks, 4), dtype=torch.float64, device=prop.device) if nblocks else None
    prop._remember_nac(pot)
    prop.synchronize()
    t = time.perf_counter()
    prop.run(pot, dt, nt, slots=slots, blocks=blocks)
    prop.synchronize()
    return time.perf_counter() - t


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "blocks_timing.jsonl")
    nblocks = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    rows = []
    for label, name, n, nt in CASES:
        g = cases.load(name)
        res, runs = {}, {}
        for b in (0, nblocks):
            one(g, min(n, 1000), 4, b)
            runs[b] = [one(g, n, nt, b) for _ in range(3)]
            res[b] = float(np.median(runs[b]))
        row = {"case": label, "fixture": name, "n": n, "steps": nt, "blocks": nblocks, "ms_per_step_plain": 1e3 * res[0] / nt,
               "ms_per_step_blocks": 1e3 * res[nblocks] / nt, "overhead_pct": 100.0 * (res[nblocks] / res[0] - 1.0),
               "ms_per_step_plain_runs": [1e3 * t / nt for t in runs[0]], "ms_per_step_blocks_runs": [1e3 * t / nt for t in runs[nblocks]]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
