#!/usr/bin/env python
"""Time of one HermanKlukPropagator.reduced_density call next to one norm() on the same state.

    python tools/density_timing.py [out.jsonl] [--cases D:n:M:ns ...] [--reps R]

Cases: Morse AS models (semiclassical_amd.synthetic.anharmonic_as_model) of D modes with n trajectories, M mode directions and a
uniform grid of ns points over the ensemble's range along mode 0; the default is the 60-mode headline model at n = 1e4, M = 1,
ns = 256.  In one process per case: initial conditions on the device, three steps, warm-up, then HIP events on the launch stream
around R consecutive calls of each (every call also packs its operands on the device and ends with a copy to the host, so the
span is the time a caller waits).  ``kernel_timing`` brackets the two launches of sc_density_pair_sum alone.  A row is appended
per case: ms per call, the pair sum's exponentials per second (n^2 M ns complex exponentials per call)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import potentials as P, propagators as PR, synthetic  # noqa: E402

STEP_AU = 4.0


def span_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def one(D, n, M, ns, reps):
    omega, chi, nac, q0, _ = synthetic.anharmonic_as_model(D)
    G = torch.diag(omega)
    pot = P.MorsePotential(omega, chi, nac)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    for _ in range(3):
        prop.step(pot, STEP_AU)
    q0s = prop.current_positions_and_momenta()[0][0]
    sigma = float(1.0 / torch.sqrt(2.0 * omega[0]))
    s = np.linspace(float(q0s.min()) - 4.0 * sigma, float(q0s.max()) + 4.0 * sigma, ns)
    modes = list(range(M))
    density = lambda: prop.reduced_density(modes, s)
    rho, norm = density(), prop.norm()
    row = {"D": D, "n": n, "M": M, "ns": ns, "reps": reps, "norm": norm}
    if ns > 1:
        row["trapezoid_over_norm2"] = float((s[1] - s[0]) * (rho[0].sum() - 0.5 * (rho[0, 0] + rho[0, -1])) / norm ** 2)
    row["ms_per_norm"] = span_ms(prop.norm, reps)
    row["ms_per_density"] = span_ms(density, reps)
    prop.kernel_timing = True
    for _ in range(reps):
        density()
    kernel = prop.kernel_times_ms()["reduced_density"]
    row["ms_per_density_kernels"] = float(np.mean(kernel))
    row["density_over_norm"] = row["ms_per_density"] / row["ms_per_norm"]
    row["gexp_per_s"] = float(n) * n * M * ns / row["ms_per_density_kernels"] * 1e-6
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "density_timing.jsonl"))
    ap.add_argument("--cases", nargs="*", default=["60:10000:1:256"])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for case in a.cases:
        D, n, M, ns = (int(x) for x in case.split(":"))
        row = one(D, n, M, ns, a.reps)
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
