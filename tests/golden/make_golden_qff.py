#!/usr/bin/env python
"""Golden vector of the quartic force field, produced by running the REFERENCE's own HermanKlukPropagator (build container only; see
make_golden.py for the compatibility aliases) on THIS package's QuarticForceFieldPotential -- the reference has no such surface, its
propagator takes any object with its potential protocol and calls the class's torch code.  Only arrays are stored.

    python tests/golden/make_golden_qff.py

  hk_qff6.npz   synthetic.qff_model(6, SEED), 64 trajectories, 20 steps of the model's dt: inputs zi, probi; outputs C(t), k_ic(t) and
                the final y (all rows, all trajectories)
"""
import logging
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, "..", ".."))

torch.set_default_dtype(torch.float64)
torch.symeig = lambda A, eigenvectors=True, upper=True: tuple(torch.linalg.eigh(A, UPLO='U' if upper else 'L'))
torch.solve = lambda B, A: (torch.linalg.solve(A, B), None)
logging.disable(logging.CRITICAL)

from semiclassical.propagators import HermanKlukPropagator          # noqa: E402
from semiclassical_amd import synthetic                             # noqa: E402

SEED, N, NT = 0, 64, 20


def main():
    m = synthetic.qff_model(6, SEED)
    pot = synthetic.qff_potential(m)
    G, q0 = torch.from_numpy(m["Gamma_0"]), torch.from_numpy(m["q0"])
    E0, dt = float(m["zero_point_energy"]), float(m["dt"])
    torch.manual_seed(0)
    prop = HermanKlukPropagator(G, G)
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=N)
    zi, probi = prop.zi.numpy().copy(), prop.probi.numpy().copy()
    C, k = np.zeros(NT, dtype=complex), np.zeros(NT, dtype=complex)
    for t in range(NT):
        C[t] = prop.autocorrelation(E0)
        k[t] = prop.ic_correlation(pot, energy0_es=E0)
        prop.step(pot, dt)
    path = os.path.join(HERE, "hk_qff6.npz")
    np.savez_compressed(path, seed=SEED, dt=dt, nt=NT, E0=E0, zi=zi, probi=probi, C=C, k=k, y=prop.y.numpy().copy())
    print(f"hk_qff6: C[-1] = {C[-1]:.6f}, |C[-1] - C[0]| = {abs(C[-1] - C[0]):.3f}, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
