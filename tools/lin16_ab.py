#!/usr/bin/env python
"""Timings of the constant-Hessian register kernels for an A/B of two libraries (GPU box): one JSON line per call with, for the
library in SC_LIB_PATH (default: the product), methylium HK at n = 1e5 as step() per step, run() at 200 steps with the product with
Phi and in normal-mode coordinates, and run() at 200 steps of the hashed (12, 7) dense shape in normal modes and of the (9, 9)
diagonal shape (tests/lin16_inputs.py).  Alternate the calls: parent, new, parent, new, ...

    SC_LIB_PATH=$PWD/var/libsc_parent.so python tools/lin16_ab.py [ntraj]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases, lin16_inputs as lin  # noqa: E402
from tests.engine_cases import engine_potential  # noqa: E402
from semiclassical_amd import propagators as PR  # noqa: E402

torch.set_default_dtype(torch.float64)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
NT = 200


def timed_run(prop, pot, dt, E0, frm):
    prop.normal_modes_from = frm
    prop.run(pot, dt, 20, E0)
    prop.synchronize()
    t0 = time.perf_counter()
    prop.run(pot, dt, NT, E0)
    prop.synchronize()
    return (time.perf_counter() - t0) / NT * 1e3


g = cases.load("hk_methylium")
pot, G0, q0, dt, E0 = engine_potential(g), cases.T(g["Gamma_0"]), cases.T(g["q0"]), float(g["dt"]), float(g["E0"])
row = {"lib": os.path.basename(os.environ.get("SC_LIB_PATH", "product")), "n": n}
prop = PR.HermanKlukPropagator(G0, G0, device="cuda")
prop.initial_conditions(q0, 0.0 * q0, G0, ntraj=n, seed=5)
for _ in range(5):
    prop.step(pot, dt)
prop.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(50):
    prop.step(pot, dt)
e1.record()
prop.synchronize()
row["methylium_step_ms"] = e0.elapsed_time(e1) / 50
row["methylium_run_phi_ms"] = timed_run(prop, pot, dt, E0, 10 ** 9)
row["methylium_run_modal_ms"] = timed_run(prop, pot, dt, E0, 16)
for key, shape, frm in (("d12_dp7_run_modal_ms", (12, 7, False), 16), ("d9_diag_run_phi_ms", (9, 9, True), 10 ** 9)):
    args, origin, G, q0h, _ = lin.model(shape)
    from semiclassical_amd import potentials as P
    hpot = P.MolecularHarmonicPotential.from_arrays(*args, origin=origin)
    G = torch.from_numpy(G)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(torch.from_numpy(q0h), torch.zeros(shape[0]), G, ntraj=n, seed=5)
    assert prop._whole_loop_applies(prop._potential_descriptor(hpot, lin.DT))
    row[key] = timed_run(prop, hpot, lin.DT, lin.E0, frm)
print(json.dumps(row), flush=True)
