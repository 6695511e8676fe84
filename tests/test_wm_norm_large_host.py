"""WM norm() beyond 16 non-zero width modes, without a GPU: the oracle against the reference's values
(tests/golden/make_golden_wm_norm_large.py) and the resources of the wide pair-sum kernel in the built library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import norm_oracle
from tests import cases

torch.set_default_dtype(torch.float64)      # the oracle follows the reference's global default (cli.py:121)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LARGE = [("wm_as24", "as24"), ("wm_as60", "as60"), ("wm_coumarin_harmonic", "cou")]


@pytest.mark.parametrize("name,tag", LARGE)
def test_oracle_reproduces_the_reference(name, tag):
    g, ref = cases.load(name), cases.load("wm_norms_large")
    pot, prop = cases.oracle_potential(g), cases.oracle_propagator(g)
    x = ref[f"{tag}_xgrid"]
    assert abs(norm_oracle.wm_norm(prop) - float(ref[f"{tag}_norm_0"])) < 1e-10 * float(ref[f"{tag}_norm_0"])
    assert cases.rel_err(norm_oracle.wm_coefficients(prop).numpy(), ref[f"{tag}_coeff_0"]) < 1e-10
    assert cases.rel_err(norm_oracle.wm_wavefunction(prop, x), ref[f"{tag}_psi_0"]) < 1e-10
    n = int(ref[f"{tag}_nsteps"])
    for _ in range(n):
        prop.step(pot, float(g["dt"]))
    want = float(ref[f"{tag}_norm_{n}"])
    assert abs(norm_oracle.wm_norm(prop) - want) < 1e-10 * want
    assert cases.rel_err(norm_oracle.wm_coefficients(prop).numpy(), ref[f"{tag}_coeff_{n}"]) < 1e-10
    assert cases.rel_err(norm_oracle.wm_wavefunction(prop, x), ref[f"{tag}_psi_{n}"]) < 1e-10


def test_golden_widths_have_more_than_16_modes():
    """the fixtures exercise the new route: d' > 16 for every case"""
    for name, _ in LARGE:
        g = cases.load(name)
        e = np.linalg.eigvalsh(g["Gamma_i"])
        assert int(np.count_nonzero(np.abs(e) > 1e-8)) > 16


def test_wide_pair_sum_kernel_needs_no_scratch_and_does_not_spill():
    lib = os.path.join(ROOT, "semiclassical_amd", "libsemiclassical_hip.so")
    assert os.path.exists(lib), "build() first"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), lib, "wm_pair_sum_wide"],
                         capture_output=True, text=True, check=True).stdout
    rows = [r for r in out.splitlines() if "wm_pair_sum_wide_kernel" in r]
    assert rows, out
    for r in rows:
        scratch = re.search(r"scratch\s+(\d+) B", r)
        spills = re.search(r"spill v (\d+) s (\d+)", r)
        assert scratch and int(scratch.group(1)) == 0, r
        assert spills and spills.group(1) == "0" and spills.group(2) == "0", r
