#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() on a thermal ensemble with M pairs of quadratic operators of rank R (thermal
correlation functions with quadratic operators).

    python tools/thermal_opquad_timing.py [out.jsonl] [--case as:60 | coumarin] [--n N] [--kelvin T]
                                          [--operators 0:0 3:1 3:60 16:2 64:1] [--steps NT] [--reps R]

The cases of tools/thermal_timing.py: ``as:D``, the Morse AS model of D modes with diagonal widths (default: the headline shape, 60
modes at n = 1e5), and ``coumarin`` (D = 51, dense widths, d'' = 45).  One process, one thermal ensemble.  A warm-up run() per shape,
then HIP events on the launch stream around R runs of NT steps for every shape, the shapes taken in turn inside each repetition
(alternating: a drift of the machine hits all of them alike); the operators are prepared before the bracket (once per set and
ensemble in production).  Every shape M:R comes with its yardstick, existing code: sc_hk_opcorr_thermal with M' = 64 x (the 64-column
tiles of the shape) LINEAR operators -- the same staged work over D and d''.  0:0 is run() without operators.  Afterwards
``kernel_timing`` brackets the launches of sc_hk_opquad_thermal (tile kernel + reduction) and of the yardstick alone.  One row per
shape is appended: ms per step of run() and of the yardstick's run(), its spread over the repetitions, ms per call of either and
their ratio."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semiclassical_amd import potentials as P, propagators as PR, synthetic, units  # noqa: E402
from tools.opquad_timing import tiles_of  # noqa: E402
from tools.thermal_opcorr_timing import operators_for  # noqa: E402
from tools.thermal_timing import coumarin  # noqa: E402


def quadratic_operators_for(G, M, R, rng):
    """M pairs of operators c + m.x + 1/2 x^T K x, every K symmetric of rank R with entries of the order of one, m and K inside the
    range of the widths"""
    e, V = np.linalg.eigh(G.numpy())
    inside = V[:, abs(e) > 1e-8]
    d = G.shape[0]

    def side():
        v = (rng.normal(size=(M, R, d)) / np.sqrt(d)) @ inside @ inside.T
        return rng.normal(size=M), (rng.normal(size=(M, d)) @ inside) @ inside.T, np.einsum('ar,ard,are->ade', rng.normal(size=(M, R)), v, v)
    return side(), side()


def run_ms(prop, pot, dt, nt, operators=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    kw = {}
    if operators is not None:
        buf = torch.zeros((nt, operators[0][0].shape[0], 5), dtype=torch.float64, device=prop.device)
        kw = dict(thermal_quadratic=operators, thermal_opquad=buf)
    e0.record()
    prop.run(pot, dt, nt, slots=slots, **kw)
    e1.record()
    e1.synchronize()
    prop.synchronize()
    return e0.elapsed_time(e1) / nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "thermal_opquad_timing.jsonl"))
    ap.add_argument("--case", default="as:60")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--kelvin", type=float, default=300.0)
    ap.add_argument("--operators", nargs="*", default=["0:0", "3:1", "3:60", "16:2", "64:1"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    if a.case == "coumarin":
        pot, q0, G, dt = coumarin()
    else:
        omega, chi, nac, q0, dt = synthetic.anharmonic_as_model(int(a.case.split(":")[1]))          # dt = 0.005 fs, the benchmark's
        G, pot = torch.diag(omega), P.MorsePotential(omega, chi, nac)
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.operators]
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.thermal_initial_conditions(q0, 0.0 * q0, G, pot.masses(), units.kelvin_to_hartree * a.kelvin, ntraj=a.n, seed=5)
    rng = np.random.default_rng(1)
    # what is timed: every shape, and the linear yardstick of every tile count (a set without a K takes sc_hk_opcorr_thermal)
    jobs = {}
    for M, R in shapes:
        jobs[("quad", M, R)] = quadratic_operators_for(G, M, R, rng) if M > 0 else None
        if M > 0:
            jobs.setdefault(("lin", 64 * tiles_of(M, R), 0), operators_for(G, 64 * tiles_of(M, R), rng))
    for ops in jobs.values():                              # warm-up: code objects, scratch, the layout of the blocks, g
        run_ms(prop, pot, dt, a.steps, ops)
    spans = {key: [] for key in jobs}
    for _ in range(a.reps):
        for key, ops in jobs.items():
            if ops is not None:
                # the propagator keeps ONE prepared set: prepare outside the bracket (the host's eigendecompositions, the upload
                # and g, once per set of operators and ensemble), so that run() inside it finds the set it was given
                prop._prepare_thermal_quadratic(ops)
            spans[key].append(run_ms(prop, pot, dt, a.steps, ops))
    prop.kernel_timing = True
    kernels = {}
    for key, ops in jobs.items():
        if ops is not None:
            prop.__dict__.pop("_kernel_events", None)
            run_ms(prop, pot, dt, a.steps, ops)
            kernels[key] = float(np.median(prop.kernel_times_ms()["hk_opquad_thermal" if key[0] == "quad" else "hk_opcorr_thermal"]))
    tc = prop._thermal["consts"]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for M, R in shapes:
        key = ("quad", M, R)
        row = {"case": a.case, "D": int(prop.dim), "dmodes": tc.dmodes, "n": a.n, "kelvin": a.kelvin, "M": M, "R": R, "steps": a.steps,
               "reps": a.reps, "ms_per_step": float(np.median(spans[key])), "ms_per_step_min": float(np.min(spans[key])),
               "ms_per_step_max": float(np.max(spans[key]))}
        if M > 0:
            lin = ("lin", 64 * tiles_of(M, R), 0)
            row.update(tiles=tiles_of(M, R), ms_per_opquad_thermal_call=kernels[key], yardstick_M=lin[1],
                       ms_per_opcorr_thermal_call=kernels[lin], ms_per_step_yardstick=float(np.median(spans[lin])),
                       ratio=kernels[key] / kernels[lin])
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
