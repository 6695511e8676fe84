#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() on a quartic force field (sc_qff_stage), next to the same
potential behind a wrapper that hides its device model, so that it takes the generic route (its own torch code at the four stage
points) -- how the engine ran such a surface before sc_qff_stage existed.

    python tools/qff_timing.py [out.jsonl] [--shapes D:n ...] [--steps NT] [--reps R]

synthetic.qff_model(D) with n trajectories; default shapes 24:100000 60:100000 96:10000.  One process: initial conditions on the
device, a warm-up run() per shape and route, then HIP events on the launch stream around R runs of NT steps, shapes and routes taken
in turn inside each repetition (alternating: a drift of the machine hits all of them alike).  Afterwards ``kernel_timing`` brackets
the launches alone.  One row per shape and route is appended: ms per step of run() with its spread; for the fused route also ms per
sc_qff_stage call (stage point + evaluation + slopes), ms per sc_dense_mono_step call, the FP64 rate of the product W = T.X
(2 D^3 n flop per call, a lower bound of the kernel's own rate: the call also runs the two small RK4 kernels) as a fraction of the
measured matrix-core rate (77 TFLOP/s, profiles/r4_mfma_f64.txt), and the rate at which a call writes its Hessian image
(8 n D^2 bytes)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import propagators as PR, synthetic  # noqa: E402
from semiclassical_amd._lib import lib  # noqa: E402

MFMA_F64_TFLOPS = 77.0


class Hidden(object):
    """the potential protocol and nothing else"""

    def __init__(self, pot):
        self.dimensions, self.masses, self.harmonic_approximation = pot.dimensions, pot.masses, pot.harmonic_approximation
        self.derivative_coupling_1st, self.derivative_coupling_2nd = pot.derivative_coupling_1st, pot.derivative_coupling_2nd


def run_ms(prop, pot, dt, nt):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    prop.synchronize()
    e0.record()
    prop.run(pot, dt, nt, slots=slots)
    e1.record()
    e1.synchronize()
    prop.synchronize()
    return e0.elapsed_time(e1) / nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "qff_timing.jsonl"))
    ap.add_argument("--shapes", nargs="*", default=["24:100000", "60:100000", "96:10000"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--routes", nargs="*", default=["qff", "generic"])
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    runs = {}
    for shape in a.shapes:
        D, n = (int(x) for x in shape.split(":"))
        m = synthetic.qff_model(D, 0)
        pot = synthetic.qff_potential(m)
        G, q0 = torch.from_numpy(m["Gamma_0"]), torch.from_numpy(m["q0"])
        for route in a.routes:
            prop = PR.HermanKlukPropagator(G, G, device="cuda")
            prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
            # dt of the benchmark (0.005 fs): the trajectories stay where they start over any number of timed steps
            runs[(D, n, route)] = (prop, pot if route == "qff" else Hidden(pot), 0.005 / 0.02418884254)
    for prop, pot, dt in runs.values():                    # warm-up: code objects, scratch
        run_ms(prop, pot, dt, 2)
    spans = {key: [] for key in runs}
    for _ in range(a.reps):
        for key, (prop, pot, dt) in runs.items():
            spans[key].append(run_ms(prop, pot, dt, a.steps))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for key, (prop, pot, dt) in runs.items():
        D, n, route = key
        row = {"D": D, "n": n, "route": route, "tile": int(lib.sc_qff_tile()), "steps": a.steps, "reps": a.reps,
               "ms_per_step": float(np.median(spans[key])), "ms_per_step_min": float(np.min(spans[key])),
               "ms_per_step_max": float(np.max(spans[key]))}
        if route == "qff":
            prop.kernel_timing = True
            run_ms(prop, pot, dt, a.steps)
            times = prop.kernel_times_ms()
            stage = float(np.median(times["qff_stage"]))
            row["ms_per_stage_call"] = stage
            row["ms_per_mono_call"] = float(np.median(times["dense_mono_step"]))
            row["gemm_tflops"] = 2.0 * D ** 3 * n / stage * 1e-9
            row["gemm_fraction_of_mfma_rate"] = row["gemm_tflops"] / MFMA_F64_TFLOPS
            row["hessian_bytes_per_call"] = 8 * n * D * D
            row["hessian_write_tb_per_s"] = 8.0 * n * D * D / stage * 1e-9
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
