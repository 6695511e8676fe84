#!/usr/bin/env python
"""Timing of the normal-mode HK step (sc_hk_step_modal) on constant-Hessian molecules of 17 to 64 modes.

    python tools/harmonic_timing.py coumarin [--wm] [--n N] [--steps K] [--warmup W]
    python tools/harmonic_timing.py ab --dims 24 33 [--n N] [--steps K]

coumarin: MolecularHarmonicPotential(S1, S1) from tests/golden/fchk, the wavepacket of the S0 ground state (D = 51, d' = 45);
run() per step from HIP events around the whole loop, kernel durations per label (HermanKlukPropagator.kernel_timing, a
separate run), and the computed floors of the step (HBM, FP64 MFMA) with the achieved fractions.
ab: random SPD Hessian with a dense rank-deficient width (d' = D - 6) -- the modal step against the Cartesian LDS kernel of
sc_hk_step (the path of the parent commit at these D), same initial conditions, ms per step and max |C difference|.
Kernel durations of record come from a separate rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import potentials as P, propagators as PR, readers  # noqa: E402
from semiclassical_amd._lib import EngineError  # noqa: E402

HBM_TBS, MFMA_TFS = 6.3, 77.0            # MI355X_MICROARCH copy rate, profiles/r4_mfma_f64.txt
FCHK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fchk")


def coumarin():
    f = {}
    for name in ("coumarin_s0", "coumarin_s1"):
        with open(os.path.join(FCHK, name + ".fchk")) as fh:
            f[name] = readers.FormattedCheckpointFile(fh)
    pot = P.MolecularHarmonicPotential(f["coumarin_s1"], f["coumarin_s1"])
    centre, widths, _ = f["coumarin_s0"].vibrational_groundstate()
    return pot, torch.from_numpy(centre), torch.from_numpy(widths)


def random_case(D, seed=7):
    rng = np.random.default_rng(seed)
    masses = rng.uniform(1800.0, 22000.0, D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    om = rng.uniform(500, 3000, D) / 219474.63
    sm = np.sqrt(masses)
    hess0 = (Q * om ** 2) @ Q.T * np.outer(sm, sm)
    hess0 = 0.5 * (hess0 + hess0.T)
    pot = P.MolecularHarmonicPotential.from_arrays(np.zeros(D), np.float64(0.0), np.zeros(D), hess0, masses, rng.normal(0, 1e-2, D))
    w = om * rng.uniform(0.7, 1.4, D)
    w[:6] = 0.0
    U, _ = np.linalg.qr(rng.standard_normal((D, D)))
    G = (U * w) @ U.T * np.outer(sm, sm)
    return pot, torch.from_numpy(rng.normal(0, 0.05, D)), torch.from_numpy(0.5 * (G + G.T))


def make(pot, q0, G, n, wm=False, modal=True):
    prop = (PR.WaltonManolopoulosPropagator(G, G, 100.0, 100.0, device="cuda") if wm
            else PR.HermanKlukPropagator(G, G, device="cuda"))
    if not modal:
        prop.modal_step_dims = (0, 0)
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, seed=5)
    return prop


def timed_run(prop, pot, dt, steps, warmup):
    prop.run(pot, dt, warmup)
    prop.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    c, _ = prop.run(pot, dt, steps)
    e1.record()
    prop.synchronize()
    return e0.elapsed_time(e1) / steps, c


def floors(D, dp, n):
    hbm = (64 * D * D + 64 * D + 72) * n / (HBM_TBS * 1e12) * 1e3
    mfma = (8 * D * D * dp + 8 * D * dp * dp) * n / (MFMA_TFS * 1e12) * 1e3
    return {"hbm_floor_ms": hbm, "mfma_floor_ms": mfma}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["coumarin", "ab"])
    ap.add_argument("--wm", action="store_true")
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="*", default=[24, 33])
    ap.add_argument("--dt", type=float, default=10.0)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    if a.what == "coumarin":
        pot, q0, G = coumarin()
        prop = make(pot, q0, G, a.n, wm=a.wm)
        ms, _ = timed_run(prop, pot, a.dt, a.steps, a.warmup)
        rec = {"case": "coumarin", "propagator": "WM" if a.wm else "HK", "n": a.n, "D": prop.dim, "dprime": prop._pre.dprime,
               "steps": a.steps, "ms_per_step": ms}
        prop.kernel_timing = True
        prop.run(pot, a.dt, 5)
        rec["kernel_ms"] = {k: float(np.median(v)) for k, v in prop.kernel_times_ms().items()}
        rec["modal"] = "hk_step_modal" in rec["kernel_ms"]          # observed: the labelled launches of the timed run
        f = floors(prop.dim, prop._pre.dprime, a.n)
        rec.update(f)
        step = rec["kernel_ms"].get("hk_step_modal")
        if step:
            rec["step_kernel_vs_hbm_floor"] = f["hbm_floor_ms"] / step
            rec["step_kernel_vs_mfma_floor"] = f["mfma_floor_ms"] / step
        print(json.dumps(rec))
        return
    for D in a.dims:
        pot, q0, G = random_case(D)
        out = {}
        for modal in (True, False):
            prop = make(pot, q0, G, a.n, modal=modal)
            try:
                out[modal] = timed_run(prop, pot, 4.0, a.steps, a.warmup)
            except EngineError as err:           # the Cartesian LDS kernel refuses D >= 34 (LDS)
                out[modal] = (None, None, str(err))
            del prop
            torch.cuda.empty_cache()
        rec = {"case": "ab", "D": D, "dprime": D - 6, "n": a.n, "steps": a.steps, "modal_ms_per_step": out[True][0],
               "coverage_ms_per_step": out[False][0]}
        if out[False][0] is None:
            rec["coverage"] = out[False][2]
        else:
            rec["max_rel_C_difference"] = float(np.max(np.abs(out[True][1] - out[False][1])) / np.max(np.abs(out[False][1])))
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
