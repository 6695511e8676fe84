#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() on a thermal ensemble with M pairs of linear operators (thermal operator correlation
functions), and of the tile call alone against its zero-temperature sibling.

    python tools/thermal_opcorr_timing.py [out.jsonl] [--case as:60 | coumarin] [--n N] [--kelvin T] [--operators 0 3 16 64]
                                          [--steps NT] [--reps R]

The cases of tools/thermal_timing.py: ``as:D``, the Morse AS model of D modes with diagonal widths (default: the headline shape, 60
modes at n = 1e5), and ``coumarin`` (D = 51, dense widths, d'' = 45).  One process, two propagators with the same seed: a thermal
ensemble for run(thermal_operators=...) and a zero-temperature one for run(operators=...) with the same operators, every vector m
projected onto the range of the widths.  A warm-up run() per M, then HIP events on the launch stream around R runs of NT steps of
the thermal propagator for every M, the values of M taken in turn inside each repetition (alternating: a drift of the machine hits
all of them alike); M = 0 is run() without operators.  Afterwards ``kernel_timing`` brackets the launches of sc_hk_opcorr_thermal
and of sc_hk_opcorr alone (tile kernel + reduction each) at the same (n, M, D).  One row per M is appended: ms per step of run(),
its spread over the repetitions, ms per call of either kernel, their ratio and the expectation (D + d'') / D."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semiclassical_amd import potentials as P, propagators as PR, synthetic, units  # noqa: E402
from tools.thermal_timing import coumarin  # noqa: E402


def operators_for(G, M, rng):
    """M pairs of operators c + m.x with entries of the order of one, every m inside the range of the widths"""
    e, V = np.linalg.eigh(G.numpy())
    inside = V[:, abs(e) > 1e-8]
    m = lambda: (rng.normal(size=(M, G.shape[0])) @ inside) @ inside.T
    return (rng.normal(size=M), m()), (rng.normal(size=M), m())


def run_ms(prop, pot, dt, nt, operators=None, thermal=True):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    kw = {}
    if operators is not None:
        buf = torch.zeros((nt, operators[0][0].shape[0], 5), dtype=torch.float64, device=prop.device)
        kw = dict(thermal_operators=operators, thermal_opcorr=buf) if thermal else dict(operators=operators, opcorr=buf)
    e0.record()
    prop.run(pot, dt, nt, slots=slots, **kw)
    e1.record()
    e1.synchronize()
    prop.synchronize()
    return e0.elapsed_time(e1) / nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "thermal_opcorr_timing.jsonl"))
    ap.add_argument("--case", default="as:60")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--kelvin", type=float, default=300.0)
    ap.add_argument("--operators", nargs="*", type=int, default=[0, 3, 16, 64])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    if a.case == "coumarin":
        pot, q0, G, dt = coumarin()
    else:
        omega, chi, nac, q0, dt = synthetic.anharmonic_as_model(int(a.case.split(":")[1]))          # dt = 0.005 fs, the benchmark's
        G, pot = torch.diag(omega), P.MorsePotential(omega, chi, nac)
    hot, cold = PR.HermanKlukPropagator(G, G, device="cuda"), PR.HermanKlukPropagator(G, G, device="cuda")
    hot.thermal_initial_conditions(q0, 0.0 * q0, G, pot.masses(), units.kelvin_to_hartree * a.kelvin, ntraj=a.n, seed=5)
    cold.initial_conditions(q0, 0.0 * q0, G, ntraj=a.n, seed=5)
    rng = np.random.default_rng(1)
    operators = {M: (operators_for(G, M, rng) if M > 0 else None) for M in a.operators}
    for M in a.operators:                                 # warm-up: code objects, scratch, the layout of the blocks, g
        run_ms(hot, pot, dt, a.steps, operators[M])
    spans = {M: [] for M in a.operators}
    for _ in range(a.reps):
        for M in a.operators:
            spans[M].append(run_ms(hot, pot, dt, a.steps, operators[M]))
    kernels = {}
    for prop, thermal, label in ((hot, True, "hk_opcorr_thermal"), (cold, False, "hk_opcorr")):
        for M in a.operators:
            if M > 0:
                prop.kernel_timing = False
                run_ms(prop, pot, dt, a.steps, operators[M], thermal)
                prop.kernel_timing = True
                prop.__dict__.pop("_kernel_events", None)
                run_ms(prop, pot, dt, a.steps, operators[M], thermal)
                kernels[label, M] = float(np.median(prop.kernel_times_ms()[label]))
    tc = hot._thermal["consts"]
    D = int(hot.dim)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for M in a.operators:
        row = {"case": a.case, "D": D, "dmodes": tc.dmodes, "n": a.n, "kelvin": a.kelvin, "M": M, "steps": a.steps, "reps": a.reps,
               "ms_per_step": float(np.median(spans[M])), "ms_per_step_min": float(np.min(spans[M])),
               "ms_per_step_max": float(np.max(spans[M]))}
        if M > 0:
            row["ms_per_opcorr_thermal_call"], row["ms_per_opcorr_call"] = kernels["hk_opcorr_thermal", M], kernels["hk_opcorr", M]
            row["call_ratio"] = row["ms_per_opcorr_thermal_call"] / row["ms_per_opcorr_call"]
            row["expected_ratio"] = (D + tc.dmodes) / D
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
