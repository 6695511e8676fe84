#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() with M pairs of quadratic operators of rank R.

    python tools/opquad_timing.py [out.jsonl] [--shape D:n] [--operators 3:1 3:60 16:2 64:1] [--steps NT] [--reps R]

The Morse AS model (semiclassical_amd.synthetic.anharmonic_as_model) of D modes with n trajectories; the default is the headline
shape, 60 modes at n = 1e5.  One process: initial conditions on the device, a warm-up run() per shape, then HIP events on the launch
stream around R runs of NT steps for every shape, the shapes taken in turn inside each repetition (alternating: a drift of the
machine hits all of them alike); the operators are prepared before the bracket (once per set and ensemble in production).  Every
shape M:R comes with its yardstick, sc_hk_opcorr with M' = 64 x (the 64-column tiles of the shape) LINEAR operators: the same d-loop
work.  0:0 is run() without operators.  Afterwards ``kernel_timing`` brackets the launches of sc_hk_opquad (tile kernel +
reduction) and of the yardstick alone.  One row per shape is appended: ms per step of run() and of the yardstick's run(),
its spread over the repetitions, ms per sc_hk_opquad call, ms per call of the yardstick and their ratio."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import potentials as P, propagators as PR, synthetic  # noqa: E402
from tools.opcorr_timing import operators_for, run_ms  # noqa: E402


def tiles_of(M, R):
    """the 64-column tiles sc_hk_opquad stages per band for M operators of 1 + R columns"""
    cols = 1 + R
    return -(-M // (64 // cols)) if cols <= 64 else M * -(-cols // 64)


def quadratic_operators_for(prop, M, R, rng):
    """M pairs of operators c + m.x + 1/2 x^T K x, every K symmetric of rank R with entries of the order of one"""
    d = prop.dim
    def side():
        v = rng.normal(size=(M, R, d)) / np.sqrt(d)
        return rng.normal(size=M), rng.normal(size=(M, d)), np.einsum('ar,ard,are->ade', rng.normal(size=(M, R)), v, v)
    return side(), side()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "opquad_timing.jsonl"))
    ap.add_argument("--shape", default="60:100000")
    ap.add_argument("--operators", nargs="*", default=["0:0", "3:1", "3:60", "16:2", "64:1"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    D, n = (int(x) for x in a.shape.split(":"))
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.operators]
    omega, chi, nac, q0, dt = synthetic.anharmonic_as_model(D)          # dt = 0.005 fs, the benchmark's
    G = torch.diag(omega)
    pot = P.MorsePotential(omega, chi, nac)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    rng = np.random.default_rng(1)
    # what is timed: every shape, and the linear yardstick of every tile count
    jobs = {}
    for M, R in shapes:
        jobs[("quad", M, R)] = quadratic_operators_for(prop, M, R, rng) if M > 0 else None
        if M > 0:
            jobs.setdefault(("lin", 64 * tiles_of(M, R), 0), operators_for(prop, 64 * tiles_of(M, R), rng))
    for ops in jobs.values():                              # warm-up: code objects, scratch, the layout of the blocks, g
        run_ms(prop, pot, dt, a.steps, ops)
    spans = {key: [] for key in jobs}
    for _ in range(a.reps):
        for key, ops in jobs.items():
            if ops is not None:
                # the propagator keeps ONE prepared set: prepare outside the bracket (the host's eigendecompositions, the upload
                # and g, once per set of operators and ensemble), so that run() inside it finds the set it was given
                prop._prepare_operators(ops)
            spans[key].append(run_ms(prop, pot, dt, a.steps, ops))
    prop.kernel_timing = True
    kernels = {}
    for key, ops in jobs.items():
        if ops is not None:
            prop.__dict__.pop("_kernel_events", None)
            run_ms(prop, pot, dt, a.steps, ops)
            kernels[key] = float(np.median(prop.kernel_times_ms()["hk_opquad" if key[0] == "quad" else "hk_opcorr"]))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for M, R in shapes:
        key = ("quad", M, R)
        row = {"D": D, "n": n, "M": M, "R": R, "steps": a.steps, "reps": a.reps, "ms_per_step": float(np.median(spans[key])),
               "ms_per_step_min": float(np.min(spans[key])), "ms_per_step_max": float(np.max(spans[key]))}
        if M > 0:
            lin = ("lin", 64 * tiles_of(M, R), 0)
            row.update(tiles=tiles_of(M, R), ms_per_opquad_call=kernels[key], yardstick_M=lin[1], ms_per_opcorr_call=kernels[lin],
                       ms_per_step_yardstick=float(np.median(spans[lin])), ratio=kernels[key] / kernels[lin])
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
