#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() with M pairs of linear operators (operator correlation functions).

    python tools/opcorr_timing.py [out.jsonl] [--shape D:n] [--operators 0 3 16 64] [--steps NT] [--reps R] [--cross-targets K]

The Morse AS model (semiclassical_amd.synthetic.anharmonic_as_model) of D modes with n trajectories; the default is the headline
shape, 60 modes at n = 1e5.  One process: initial conditions on the device, a warm-up run() per M, then HIP events on the launch
stream around R runs of NT steps for every M, the values of M taken in turn inside each repetition (alternating: a drift of the
machine hits all of them alike).  M = 0 is run() without operators.  Afterwards ``kernel_timing`` brackets the launches of
sc_hk_opcorr alone (tile kernel + reduction).  One row per M is appended: ms per step of run(), its spread over the repetitions,
ms per sc_hk_opcorr call, and the pair rate n M / time of the kernels.  The yardstick of the call, sc_hk_cross with K targets (16)
on the same state in the same session, closes the file as a row of its own ("K" instead of "M")."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import potentials as P, propagators as PR, synthetic  # noqa: E402
from tools.cross_timing import targets_for  # noqa: E402


def operators_for(prop, M, rng):
    """M pairs of operators c + m.x with entries of the order of one"""
    d = prop.dim
    return (rng.normal(size=M), rng.normal(size=(M, d))), (rng.normal(size=M), rng.normal(size=(M, d)))


def run_ms(prop, pot, dt, nt, operators=None, targets=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    kw = {}
    if operators is not None:
        kw = dict(operators=operators, opcorr=torch.zeros((nt, operators[0][0].shape[0], 5), dtype=torch.float64, device=prop.device))
    if targets is not None:
        kw = dict(targets=targets, cross=torch.zeros((nt, targets[0].shape[0], 5), dtype=torch.float64, device=prop.device))
    e0.record()
    prop.run(pot, dt, nt, slots=slots, **kw)
    e1.record()
    e1.synchronize()
    prop.synchronize()
    return e0.elapsed_time(e1) / nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "opcorr_timing.jsonl"))
    ap.add_argument("--shape", default="60:100000")
    ap.add_argument("--operators", nargs="*", type=int, default=[0, 3, 16, 64])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cross-targets", type=int, default=16)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    D, n = (int(x) for x in a.shape.split(":"))
    omega, chi, nac, q0, dt = synthetic.anharmonic_as_model(D)          # dt = 0.005 fs, the benchmark's
    G = torch.diag(omega)
    pot = P.MorsePotential(omega, chi, nac)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    rng = np.random.default_rng(1)
    operators = {M: (operators_for(prop, M, rng) if M > 0 else None) for M in a.operators}
    for M in a.operators:                                 # warm-up: code objects, scratch, the layout of the blocks, g
        run_ms(prop, pot, dt, a.steps, operators[M])
    spans = {M: [] for M in a.operators}
    for _ in range(a.reps):
        for M in a.operators:
            spans[M].append(run_ms(prop, pot, dt, a.steps, operators[M]))
    prop.kernel_timing = True
    kernels = {}
    for M in a.operators:
        if M > 0:
            prop.__dict__.pop("_kernel_events", None)
            run_ms(prop, pot, dt, a.steps, operators[M])
            kernels[M] = prop.kernel_times_ms()["hk_opcorr"]
    cross = None
    if a.cross_targets > 0:
        targets = targets_for(prop, a.cross_targets, rng)
        prop.kernel_timing = False
        run_ms(prop, pot, dt, a.steps, targets=targets)
        prop.kernel_timing = True
        prop.__dict__.pop("_kernel_events", None)
        run_ms(prop, pot, dt, a.steps, targets=targets)
        cross = prop.kernel_times_ms()["hk_cross"]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    rows = []
    for M in a.operators:
        row = {"D": D, "n": n, "M": M, "steps": a.steps, "reps": a.reps, "ms_per_step": float(np.median(spans[M])),
               "ms_per_step_min": float(np.min(spans[M])), "ms_per_step_max": float(np.max(spans[M]))}
        if M > 0:
            row["ms_per_opcorr_call"] = float(np.median(kernels[M]))
            row["gpairs_per_s"] = float(n) * M / row["ms_per_opcorr_call"] * 1e-6
        rows.append(row)
    if cross is not None:
        rows.append({"D": D, "n": n, "K": a.cross_targets, "steps": a.steps, "ms_per_cross_call": float(np.median(cross))})
    for row in rows:
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
