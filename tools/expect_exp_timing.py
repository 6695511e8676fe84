#!/usr/bin/env python
"""Time of HermanKlukPropagator.expectation(ex=...) calls and of the Morse <H> next to norm() on the same state.

    python tools/expect_exp_timing.py [out.jsonl] [--D 60] [--n 10000] [--reps 3]

The Morse AS model (semiclassical_amd.synthetic.anharmonic_as_model) of D modes with n trajectories, three steps, then four
shapes in turn, `reps` rounds with the shapes alternating, HIP events on the launch stream around every call (a call packs its
operands on the device and ends with a copy to the host, so the span is the time a caller waits):

    norm         norm()
    constant     expectation(c=[1], ex=(w (1, 0), a (1, 0, D))): the constant alone through sc_pair_expect_exp, P = 0
    exponential  expectation(ex=...) of exp(-a_0 x_0): one product column
    morse_H      anharmonic_energy_expectation(potential): R = D squared p-columns and P = 2 D product columns in one operator

``kernel_timing`` brackets the two launches of sc_pair_expect_exp alone.  One row per shape is appended: the ms of every round,
their median, the median over norm()'s, and the ms of the launches."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import potentials as P, propagators as PR, synthetic  # noqa: E402

STEP_AU = 4.0


def span_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "expect_exp_timing.jsonl"))
    ap.add_argument("--D", type=int, default=60)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    D, n = a.D, a.n
    omega, chi, nac, q0, _ = synthetic.anharmonic_as_model(D)
    G = torch.diag(omega)
    pot = P.MorsePotential(omega, chi, nac)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    for _ in range(3):
        prop.step(pot, STEP_AU)
    one = np.zeros((1, 1, D))
    one[0, 0, 0] = float(pot.a[0])
    shapes = {
        "norm": (prop.norm, 0, 0, 0),
        "constant": (lambda: prop.expectation(c=np.ones(1), ex=(np.zeros((1, 0)), np.zeros((1, 0, D)))), 1, 0, 0),
        "exponential": (lambda: prop.expectation(ex=(np.ones((1, 1)), one)), 1, 0, 1),
        "morse_H": (lambda: prop.anharmonic_energy_expectation(pot), 1, D, 2 * D),
    }
    values = {k: fn() for k, (fn, _, _, _) in shapes.items()}              # warm-up
    ms = {k: [] for k in shapes}
    for _ in range(a.reps):
        for k, (fn, _, _, _) in shapes.items():
            ms[k].append(span_ms(fn))
    prop.kernel_timing = True
    kernels = {}
    for k, (fn, _, _, _) in shapes.items():
        if k != "norm":
            before = len(prop.__dict__.get("_kernel_events", {}).get("expectation", []))
            fn()
            kernels[k] = float(prop.kernel_times_ms()["expectation"][before])
    prop.kernel_timing = False
    norm_ms = float(np.median(ms["norm"]))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        for k, (_, M, R, Pc) in shapes.items():
            row = {"D": D, "n": n, "shape": k, "M": M, "R": R, "P": Pc, "ms": ms[k], "ms_median": float(np.median(ms[k])),
                   "over_norm": float(np.median(ms[k])) / norm_ms}
            if k in kernels:
                row["ms_kernels"] = kernels[k]
            if k == "morse_H":
                row["value"] = float(values[k])
            print(json.dumps(row), flush=True)
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
