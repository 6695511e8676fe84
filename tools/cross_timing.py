#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() with K target coherent states (cross-correlation functions).

    python tools/cross_timing.py [out.jsonl] [--shape D:n] [--targets 0 16 64 256] [--steps NT] [--reps R]

The Morse AS model (semiclassical_amd.synthetic.anharmonic_as_model) of D modes with n trajectories; the default is the headline
shape, 60 modes at n = 1e5.  One process: initial conditions on the device, a warm-up run() per K, then HIP events on the launch
stream around R runs of NT steps for every K, the values of K taken in turn inside each repetition (alternating: a drift of the
machine hits all of them alike).  K = 0 is run() without targets.  Afterwards ``kernel_timing`` brackets the launches of
sc_hk_cross alone (tile kernel + reduction, for dense widths also the operand pre-pass).  One row per K is appended: ms per step
of run(), its spread over the repetitions, ms per sc_hk_cross call, and the pair rate n K / time of the cross kernels."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import potentials as P, propagators as PR, synthetic  # noqa: E402

def targets_for(prop, K, rng):
    """K targets around (q0, p0), within a tenth of a width per mode: overlaps of the order of one"""
    d = prop.dim
    q0, p0, g = prop._q0h.numpy(), prop._p0h.numpy(), torch.diagonal(prop._G0h).numpy()
    return (q0 + 0.1 * rng.uniform(-1.0, 1.0, (K, d)) / np.sqrt(g), p0 + 0.1 * rng.uniform(-1.0, 1.0, (K, d)) * np.sqrt(g))


def run_ms(prop, pot, dt, nt, targets):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    kw = {}
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
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "cross_timing.jsonl"))
    ap.add_argument("--shape", default="60:100000")
    ap.add_argument("--targets", nargs="*", type=int, default=[0, 16, 64, 256])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    D, n = (int(x) for x in a.shape.split(":"))
    omega, chi, nac, q0, dt = synthetic.anharmonic_as_model(D)          # dt = 0.005 fs, the benchmark's
    G = torch.diag(omega)
    pot = P.MorsePotential(omega, chi, nac)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    rng = np.random.default_rng(1)
    targets = {K: (targets_for(prop, K, rng) if K > 0 else None) for K in a.targets}
    for K in a.targets:                                   # warm-up: code objects, scratch, the layout of the blocks
        run_ms(prop, pot, dt, a.steps, targets[K])
    spans = {K: [] for K in a.targets}
    for _ in range(a.reps):
        for K in a.targets:
            spans[K].append(run_ms(prop, pot, dt, a.steps, targets[K]))
    prop.kernel_timing = True
    kernels = {}
    for K in a.targets:
        if K > 0:
            prop.__dict__.pop("_kernel_events", None)
            run_ms(prop, pot, dt, a.steps, targets[K])
            kernels[K] = prop.kernel_times_ms()["hk_cross"]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for K in a.targets:
        row = {"D": D, "n": n, "K": K, "steps": a.steps, "reps": a.reps, "ms_per_step": float(np.median(spans[K])),
               "ms_per_step_min": float(np.min(spans[K])), "ms_per_step_max": float(np.max(spans[K]))}
        if K > 0:
            row["ms_per_cross_call"] = float(np.median(kernels[K]))
            row["gpairs_per_s"] = float(n) * K / row["ms_per_cross_call"] * 1e-6
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
