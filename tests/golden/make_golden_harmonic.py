#!/usr/bin/env python
"""Golden vectors of coumarin on its harmonic surface, produced by running the REFERENCE itself (build container only; see
make_golden.py for the compatibility aliases and make_golden_driver.py for the `ase` stand-in).  Only arrays are stored.

    python tests/golden/make_golden_harmonic.py

  hk_coumarin_harmonic.npz      reference HK on MolecularHarmonicPotential(coumarin_s1, coumarin_s1) (D = 51), widths Gamma_0 of
                                the S0 vibrational ground state (dense, d' = 45), 64 trajectories, 20 steps of 10 au: zi, probi,
                                C(t), k_ic(t), c2 per step, final (q, p, S) and signs of all trajectories, final monodromy
                                blocks of the first NBLK trajectories (mono_final [4][D][D][NBLK])
  wm_coumarin_harmonic.npz      the same with Walton-Manolopoulos (alpha = beta = 1e4), 32 trajectories, 10 steps
  driver_coumarin_harmonic.npz  the reference's `semi dynamics` + `semi rates` on a "harmonic" task with the coumarin fchk files
                                (ground S0, excited / coupling S1; HK, 32 trajectories in batches of 16, 12 steps), stored as
                                driver_methylium.npz (the reference's outcome if its set-up raises)
The time step passes the reference's own energy check (propagators.py:385-398).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_driver as mgd          # noqa: E402  (imports the reference with the ase stand-in, defines run_reference_task)
from semiclassical import readers, units                                                 # noqa: E402
from semiclassical.potentials import MolecularHarmonicPotential                          # noqa: E402
from semiclassical.propagators import HermanKlukPropagator, WaltonManolopoulosPropagator  # noqa: E402

FCHK = os.path.join(HERE, "fchk")
NBLK = 8
DT = 10.0


def fchk(name):
    with open(os.path.join(FCHK, name + ".fchk")) as f:
        return readers.FormattedCheckpointFile(f)


def run(name, make, pot, q0, G0, E0, n, nt, extra):
    torch.manual_seed(0)
    prop = make()
    prop.initial_conditions(q0, 0.0 * q0, G0, ntraj=n)
    d = prop.dim
    cauto, kic = np.zeros(nt, dtype=complex), np.zeros(nt, dtype=complex)
    c2 = np.zeros((nt + 1, n), dtype=complex)
    c2[0] = prop.sign_trackers["prefactorC"]["previous"].numpy()
    for t in range(nt):
        cauto[t] = prop.autocorrelation(E0)
        kic[t] = prop.ic_correlation(pot, energy0_es=E0)
        prop.step(pot, DT)
        c2[t + 1] = prop.sign_trackers["prefactorC"]["previous"].numpy()
    y = prop.y.numpy()
    out = dict(extra, q0=q0.numpy(), p0=0.0 * q0.numpy(), Gamma_0=G0.numpy(), Gamma_i=prop.Gamma_i.numpy(),
               Gamma_t=prop.Gamma_t.numpy(), dt=DT, nt=nt, E0=float(E0), zi=prop.zi.numpy().copy(), probi=prop.probi.numpy().copy(),
               cauto=cauto, kic=kic, c2=c2, qpS_final=np.vstack((y[:2 * d], y[-1:])),
               mono_final=y[2 * d:2 * d + 4 * d * d, :NBLK].reshape(4, d, d, NBLK).copy(),
               signs_final=prop.sign_trackers["prefactorC"]["signs"].numpy().copy())
    if isinstance(prop, WaltonManolopoulosPropagator):
        out.update(signsA_final=prop.sign_trackers["detA"]["signs"].numpy().copy(),
                   signsM_final=prop.sign_trackers["detM"]["signs"].numpy().copy())
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name:28s} D={d} d'={prop.U.shape[1]} n={n} nt={nt} C[-1]={cauto[-1]:.6f} "
          f"flips={int((out['signs_final'].real < 0).sum())} {os.path.getsize(path) / 1024:.0f} KiB")


def dynamics():
    s0, s1 = fchk("coumarin_s0"), fchk("coumarin_s1")
    pos0, energy0, grad0, hess0 = s1.harmonic_approximation()
    pot = MolecularHarmonicPotential(s1, s1)
    x0, Gamma_0, en_zpt = s0.vibrational_groundstate()
    q0, G0 = torch.from_numpy(x0), torch.from_numpy(Gamma_0)
    ex = dict(potential="harmonic", pos0=pos0, energy0=energy0, grad0=grad0, hess0=hess0, masses=s1.masses(),
              nac0=s1.nonadiabatic_coupling(), origin=float(getattr(pot, "_origin", 0.0)))
    run("hk_coumarin_harmonic", lambda: HermanKlukPropagator(G0, G0), pot, q0, G0, en_zpt, 64, 20, ex)
    run("wm_coumarin_harmonic", lambda: WaltonManolopoulosPropagator(G0, G0, 1.0e4, 1.0e4), pot, q0, G0, en_zpt, 32, 10,
        dict(ex, alpha=1.0e4, beta=1.0e4))


def driver():
    rates = {"task": "rates", "broadening": "gaussian"}
    task = {"task": "dynamics",
            "potential": {"type": "harmonic", "ground": os.path.join(FCHK, "coumarin_s0.fchk"),
                          "excited": os.path.join(FCHK, "coumarin_s1.fchk"), "coupling": os.path.join(FCHK, "coumarin_s1.fchk")},
            "propagator": "HK", "batch_size": 16, "num_trajectories": 32, "num_steps": 12,
            "time_step_fs": DT * units.autime_to_fs, "manual_seed": 0}
    out = {"task": json.dumps({k: v for k, v in task.items() if k not in ("potential", "results")}), "rates_task": json.dumps(rates)}
    try:
        data, zis, probis = mgd.run_reference_task(task, rates)
        out.update({f"res_{k}": v for k, v in data.items()})
        out["zi"], out["probi"] = np.stack(zis), np.stack(probis)
        out["outcome"] = "ok"
        print("driver: C(0) =", data["autocorrelation"][0], "trajectories", data["trajectories"], "keys", sorted(data))
    except Exception as err:          # whatever the reference does on this input is what the driver has to do as well
        out["outcome"], out["message"] = type(err).__name__, str(err)
        print("driver:", out["outcome"], out["message"])
    np.savez_compressed(os.path.join(HERE, "driver_coumarin_harmonic.npz"), **out)


if __name__ == "__main__":
    dynamics()
    driver()
