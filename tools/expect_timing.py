#!/usr/bin/env python
"""Time of HermanKlukPropagator.expectation calls next to norm() on the same state.

    python tools/expect_timing.py [out.jsonl] [--D 60] [--n 10000] [--reps 3]

The Morse AS model (semiclassical_amd.synthetic.anharmonic_as_model) of D modes with n trajectories, three steps, then four
shapes in turn, `reps` rounds with the shapes alternating, HIP events on the launch stream around every call (a call packs its
operands on the device and ends with a copy to the host, so the span is the time a caller waits):

    norm        norm()
    constant    expectation(c=[1]): the exponent work of norm() and one operator of one column of zeros
    linear      expectation of all of <x_k> and <p_k>: 2 D operators of one column
    quadratic   expectation of one operator with full-rank xx and pp: R = 2 D squared columns

``kernel_timing`` brackets the two launches of sc_pair_expect alone.  One row per shape is appended: the ms of every round, their
median, the median over norm()'s, and the ms of the launches."""
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
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "expect_timing.jsonl"))
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
    eye, zeros = np.eye(D), np.zeros((D, D))
    rng = np.random.default_rng(1)
    sym = rng.standard_normal((2, D, D))
    sym = sym + sym.transpose(0, 2, 1)
    shapes = {
        "norm": (prop.norm, 0, 0),
        "constant": (lambda: prop.expectation(c=np.ones(1)), 1, 0),
        "linear": (lambda: prop.expectation(x=np.concatenate((eye, zeros)), p=np.concatenate((zeros, eye))), 2 * D, 0),
        "quadratic": (lambda: prop.expectation(xx=sym[:1], pp=sym[1:]), 1, 2 * D),
    }
    for fn, _, _ in shapes.values():                                    # warm-up
        fn()
    ms = {k: [] for k in shapes}
    for _ in range(a.reps):
        for k, (fn, _, _) in shapes.items():
            ms[k].append(span_ms(fn))
    prop.kernel_timing = True
    kernels = {}
    for k, (fn, _, _) in shapes.items():
        if k != "norm":
            before = len(prop.__dict__.get("_kernel_events", {}).get("expectation", []))
            fn()
            kernels[k] = float(prop.kernel_times_ms()["expectation"][before])
    prop.kernel_timing = False
    norm_ms = float(np.median(ms["norm"]))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        for k, (_, M, R) in shapes.items():
            row = {"D": D, "n": n, "shape": k, "M": M, "R": R, "ms": ms[k], "ms_median": float(np.median(ms[k])),
                   "over_norm": float(np.median(ms[k])) / norm_ms}
            if k in kernels:
                row["ms_kernels"] = kernels[k]
            print(json.dumps(row), flush=True)
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
