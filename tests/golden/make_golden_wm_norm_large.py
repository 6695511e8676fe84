#!/usr/bin/env python
"""Golden values of WaltonManolopoulosPropagator.norm() / coefficients() / wavefunction() for WM cases with more than 16
non-zero width modes, from the REFERENCE (build container only; make_golden_driver.py imports it with the `ase` stand-in).

    python tests/golden/make_golden_wm_norm_large.py

Starts from the initial conditions (zi, probi) of existing goldens, so the engine and the oracle can be started from
identical states, and stores for each case, with the prefixes as24_, as60_, cou_:
  norm_0, coeff_0, psi_0            at t = 0
  norm_<n>, coeff_<n>, psi_<n>      after nsteps steps of the golden's time step
  xgrid                             the spatial grid of wavefunction()
Cases: wm_as24 (D = d' = 24), wm_as60 (D = d' = 60), wm_coumarin_harmonic (D = 51, d' = 45).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_driver  # noqa: E402,F401  (imports the reference with the ase stand-in)
from semiclassical import readers  # noqa: E402
from semiclassical.potentials import MolecularHarmonicPotential, MorsePotential  # noqa: E402
from semiclassical.propagators import WaltonManolopoulosPropagator  # noqa: E402


def run(name, potential, nsteps):
    g = dict(np.load(os.path.join(HERE, name + ".npz")))
    T = lambda x: torch.from_numpy(np.asarray(x)).clone()
    torch.manual_seed(0)
    prop = WaltonManolopoulosPropagator(T(g["Gamma_i"]), T(g["Gamma_t"]), float(g["alpha"]), float(g["beta"]))
    prop.initial_conditions(T(g["q0"]), T(g["p0"]), T(g["Gamma_0"]), ntraj=g["zi"].shape[1])
    assert np.array_equal(prop.zi.numpy(), g["zi"])          # same seed => same initial conditions as the golden
    rng = np.random.default_rng(13)
    d = g["q0"].shape[0]
    xgrid = g["q0"][:, None] + 0.3 * rng.standard_normal((d, 9)) / np.sqrt(np.maximum(np.diag(g["Gamma_t"]), 1e-3))[:, None]
    out = {"xgrid": xgrid, "norm_0": prop.norm(), "coeff_0": prop.coefficients().numpy(), "psi_0": prop.wavefunction(T(xgrid))}
    for _ in range(nsteps):
        prop.step(potential, float(g["dt"]))
    out.update({"nsteps": nsteps, f"norm_{nsteps}": prop.norm(), f"coeff_{nsteps}": prop.coefficients().numpy(),
                f"psi_{nsteps}": prop.wavefunction(T(xgrid))})
    print(f"{name:22s} D={d} d'={prop.U.shape[1]} n={prop.ntraj} norm_0={out['norm_0']:.6e} "
          f"norm_{nsteps}={out[f'norm_{nsteps}']:.6e}")
    return out


def main():
    res = {}
    for name, tag, nsteps in (("wm_as24", "as24", 3), ("wm_as60", "as60", 2)):
        g = dict(np.load(os.path.join(HERE, name + ".npz")))
        pot = MorsePotential(torch.from_numpy(g["omega"]), torch.from_numpy(g["chi"]).clone(), torch.from_numpy(g["nac"]))
        res.update({f"{tag}_{k}": v for k, v in run(name, pot, nsteps).items()})
    with open(os.path.join(HERE, "fchk", "coumarin_s1.fchk")) as f:
        s1 = readers.FormattedCheckpointFile(f)
    pot = MolecularHarmonicPotential(s1, s1)
    res.update({f"cou_{k}": v for k, v in run("wm_coumarin_harmonic", pot, 3).items()})
    np.savez_compressed(os.path.join(HERE, "wm_norms_large.npz"), **res)


if __name__ == "__main__":
    main()
