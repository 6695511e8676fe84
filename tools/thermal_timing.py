#!/usr/bin/env python
"""Time per step of HermanKlukPropagator.run() with and without a thermal ensemble.

    python tools/thermal_timing.py [out.jsonl] [--case as:60 | coumarin] [--n N] [--kelvin T] [--steps NT] [--reps R]

``as:D``: the Morse AS model (semiclassical_amd.synthetic.anharmonic_as_model) of D modes, diagonal widths -- the default is the
headline shape, 60 modes at n = 1e5.  ``coumarin``: MolecularHarmonicPotential(S1, S1) from tests/golden/fchk with the wavepacket
of the S0 ground state (D = 51, dense widths, d'' < D).  One process, two propagators with the same seed: ``initial_conditions``
and ``thermal_initial_conditions`` on the device.  A warm-up run() each, then HIP events on the launch stream around R runs of NT
steps, the two taken in turn inside each repetition (alternating: a drift of the machine hits both alike).  Afterwards
``kernel_timing`` brackets the correlate launches alone: sc_hk_correlate_m against sc_hk_correlate_thermal.  One row is appended:
ms per step of either run(), their spread over the repetitions, their ratio, and ms per correlate launch of either kernel."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semiclassical_amd import potentials as P, propagators as PR, readers, synthetic, units  # noqa: E402


def coumarin():
    f = {}
    for name in ("coumarin_s0", "coumarin_s1"):
        with open(os.path.join(ROOT, "tests", "golden", "fchk", name + ".fchk")) as fh:
            f[name] = readers.FormattedCheckpointFile(fh)
    pot = P.MolecularHarmonicPotential(f["coumarin_s1"], f["coumarin_s1"])
    centre, widths, _ = f["coumarin_s0"].vibrational_groundstate()
    return pot, torch.from_numpy(centre), torch.from_numpy(widths), 10.0


def run_ms(prop, pot, dt, nt):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    e0.record()
    prop.run(pot, dt, nt, slots=slots)
    e1.record()
    e1.synchronize()
    prop.synchronize()
    return e0.elapsed_time(e1) / nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join("profiles", "thermal_timing.jsonl"))
    ap.add_argument("--case", default="as:60")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--kelvin", type=float, default=300.0)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    if a.case == "coumarin":
        pot, q0, G, dt = coumarin()
    else:
        omega, chi, nac, q0, dt = synthetic.anharmonic_as_model(int(a.case.split(":")[1]))          # dt = 0.005 fs, the benchmark's
        G, pot = torch.diag(omega), P.MorsePotential(omega, chi, nac)
    kT = units.kelvin_to_hartree * a.kelvin
    props = {}
    for name in ("zero", "thermal"):
        prop = PR.HermanKlukPropagator(G, G, device="cuda")
        if name == "zero":
            prop.initial_conditions(q0, 0.0 * q0, G, ntraj=a.n, seed=5)
        else:
            prop.thermal_initial_conditions(q0, 0.0 * q0, G, pot.masses(), kT, ntraj=a.n, seed=5)
        props[name] = prop
        run_ms(prop, pot, dt, a.steps)                    # warm-up: code objects, scratch, the layout of the blocks
    spans = {name: [] for name in props}
    for _ in range(a.reps):
        for name, prop in props.items():
            spans[name].append(run_ms(prop, pot, dt, a.steps))
    kernels = {}
    for name, prop in props.items():
        prop.kernel_timing = True
        prop.__dict__.pop("_kernel_events", None)
        run_ms(prop, pot, dt, a.steps)
        times = prop.kernel_times_ms()
        kernels[name] = float(np.median(times["hk_correlate_thermal" if name == "thermal" else "hk_correlate"]))
    tc = props["thermal"]._thermal["consts"]
    row = {"case": a.case, "D": int(props["zero"].dim), "dmodes": tc.dmodes, "diag": bool(tc.diag), "n": a.n, "kelvin": a.kelvin,
           "steps": a.steps, "reps": a.reps}
    for name in props:
        row[f"ms_per_step_{name}"] = float(np.median(spans[name]))
        row[f"ms_per_step_{name}_min"], row[f"ms_per_step_{name}_max"] = float(np.min(spans[name])), float(np.max(spans[name]))
        row[f"ms_per_correlate_{name}"] = kernels[name]
    row["step_ratio"] = row["ms_per_step_thermal"] / row["ms_per_step_zero"]
    row["correlate_ratio"] = kernels["thermal"] / kernels["zero"]
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
