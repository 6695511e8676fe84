#!/usr/bin/env python
"""Time of one symplecticity check (HermanKlukPropagator.symplectic_deviation) next to one HK step of the same shape.

    python tools/symplectic_timing.py [out.jsonl] [--cases D:n ...] [--reps R]

Cases: Morse AS models (semiclassical_amd.synthetic.anharmonic_as_model) of D = 12, 33, 60 modes with n = 1e5 trajectories and
D = 130 with n = 1e3.  In one process per case: initial conditions on the device, warm-up, then HIP events on the launch stream
around R consecutive steps and around R consecutive checks (the launches queue up, so the span is device time).  For 16 < D <= 64
the state is in the tiled storage order after a step; the check is timed there and again after a conversion to row-major.
A row is appended per case: ms per step / check, and the check's rate against its model of 8 D^3 flop and 32 D^2 bytes per
trajectory as fractions of the FP64 matrix pipe (profiles/r4_mfma_f64.txt) and of the HBM copy rate."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import _lib, potentials as P, propagators as PR, synthetic  # noqa: E402

HBM_TBS, MFMA_TFS = 6.3, 77.0            # MI355X copy rate, profiles/r4_mfma_f64.txt
STEP_AU = 4.0


def span_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def one(D, n, reps):
    omega, chi, nac, q0, _ = synthetic.anharmonic_as_model(D)
    G = torch.diag(omega)
    pot = P.MorsePotential(omega, chi, nac)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    step = lambda: prop.step(pot, STEP_AU)
    check = lambda: prop.symplectic_deviation(per_block=True)
    for _ in range(3):
        step()
        check()
    prop.synchronize()
    row = {"D": D, "n": n, "reps": reps, "ms_per_step": span_ms(step, reps)}
    tiled = prop._state.mono_layout == _lib.SC_MONO_TILED16
    row["layout"] = "tiled16" if tiled else "rowmajor"
    row["ms_per_check"] = span_ms(check, reps)
    eps = prop.symplectic_deviation()
    row["eps_max"], row["eps_mean"] = float(eps.max()), float(eps.mean())
    if tiled:
        prop.monodromy_matrices()              # converts the state to row-major
        check()
        row["ms_per_check_rowmajor"] = span_ms(check, reps)
    prop.synchronize()
    ms = row["ms_per_check"]
    flop, byts = 8.0 * D ** 3 * n, 32.0 * D * D * n
    row.update(check_over_step=ms / row["ms_per_step"], tflops=flop / ms * 1e-9, gbytes_per_s=byts / ms * 1e-6,
               fraction_of_mfma_rate=flop / ms * 1e-9 / MFMA_TFS, fraction_of_hbm_rate=byts / ms * 1e-9 / HBM_TBS)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "symplectic_timing.jsonl"))
    ap.add_argument("--cases", nargs="*", default=["12:100000", "33:100000", "60:100000", "130:1000"])
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for case in a.cases:
        D, n = (int(x) for x in case.split(":"))
        row = one(D, n, a.reps)
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
