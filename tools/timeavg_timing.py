#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() with a time-average accumulator (time-averaged HK spectra).

    python tools/timeavg_timing.py [out.jsonl] [--shape D:n] [--energies 0 64 512] [--steps NT] [--reps R]

The Morse AS model (semiclassical_amd.synthetic.anharmonic_as_model) of D modes with n trajectories; the default is the headline
shape, 60 modes at n = 1e5, 64 steps (two full blocks of columns).  One process: initial conditions on the device, a warm-up run()
per NE, then HIP events on the launch stream around R runs of NT steps for every NE, the values of NE taken in turn inside each
repetition (alternating: a drift of the machine hits all of them alike).  NE = 0 is run() without an accumulator; otherwise one
reference state (K = 1) and NE energies around the zero-point energy, a fresh accumulator per run, created outside the bracket.
Afterwards ``kernel_timing`` brackets the launches of sc_hk_ta_terms and sc_hk_ta_accumulate alone.  One row per NE is appended:
ms per step of run(), its spread over the repetitions, ms per terms call, ms per accumulate call (one per TB steps) and the rate
at which that call moves A (one read and one write of 16 n K NE bytes)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import potentials as P, propagators as PR, synthetic  # noqa: E402


def run_ms(prop, pot, dt, nt, energies):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    kw = {} if energies is None else dict(time_average=prop.time_average(energies, dt))
    prop.synchronize()
    e0.record()
    prop.run(pot, dt, nt, slots=slots, **kw)
    e1.record()
    e1.synchronize()
    prop.synchronize()
    return e0.elapsed_time(e1) / nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "timeavg_timing.jsonl"))
    ap.add_argument("--shape", default="60:100000")
    ap.add_argument("--energies", nargs="*", type=int, default=[0, 64, 512])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    D, n = (int(x) for x in a.shape.split(":"))
    omega, chi, nac, q0, dt = synthetic.anharmonic_as_model(D)          # dt = 0.005 fs, the benchmark's
    G = torch.diag(omega)
    pot = P.MorsePotential(omega, chi, nac)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    zpe = 0.5 * float(omega.sum())
    energies = {NE: (zpe + np.linspace(-0.01, 0.03, NE) if NE > 0 else None) for NE in a.energies}
    for NE in a.energies:                                 # warm-up: code objects, scratch, the layout of the blocks
        run_ms(prop, pot, dt, a.steps, energies[NE])
    spans = {NE: [] for NE in a.energies}
    for _ in range(a.reps):
        for NE in a.energies:
            spans[NE].append(run_ms(prop, pot, dt, a.steps, energies[NE]))
    prop.kernel_timing = True
    kernels = {}
    for NE in a.energies:
        if NE > 0:
            prop.__dict__.pop("_kernel_events", None)
            run_ms(prop, pot, dt, a.steps, energies[NE])
            times = prop.kernel_times_ms()
            kernels[NE] = (times["hk_ta_terms"], times.get("hk_ta_accumulate"))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for NE in a.energies:
        row = {"D": D, "n": n, "K": 1 if NE > 0 else 0, "NE": NE, "steps": a.steps, "reps": a.reps,
               "ms_per_step": float(np.median(spans[NE])), "ms_per_step_min": float(np.min(spans[NE])),
               "ms_per_step_max": float(np.max(spans[NE]))}
        if NE > 0:
            terms, accumulate = kernels[NE]
            row["ms_per_terms_call"] = float(np.median(terms))
            if accumulate is not None:
                row["ms_per_accumulate_call"] = float(np.median(accumulate))
                row["accumulate_tb_per_s"] = 2.0 * 16.0 * n * NE / row["ms_per_accumulate_call"] * 1e-9
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
