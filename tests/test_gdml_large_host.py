"""sGDML beyond 48 atoms without a GPU: the argument checks of sc_gdml_eval / sc_gdml_stage run before any launch, so
the accepted and refused sizes, the scratch sizing and the resources of the new kernels are checked on the host."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from semiclassical_amd._lib import lib, sc_gdml_model, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC_OK, SC_ERR_UNSUPPORTED = 0, -2


def _aligned(n):
    """16-byte aligned host buffer of n doubles (nothing is dereferenced when n = 0 geometries)"""
    raw = np.zeros(n + 2)
    off = (-raw.ctypes.data % 16) // 8
    return raw[off:off + n]


def _model(n_atoms, n_train=7):
    dd = n_atoms * (n_atoms - 1) // 2
    keep = [_aligned(n_train * dd), _aligned(n_train * dd), np.zeros(dd, np.int32), np.zeros(dd, np.int32),
            _aligned(3 * n_atoms), _aligned(64)]
    p = lambda a: C.c_void_p(a.ctypes.data)
    m = sc_gdml_model(n_atoms=n_atoms, n_desc=dd, n_train=n_train, xs_train=p(keep[0]),
                      jx_alphas=p(keep[1]), pair_k=p(keep[2]), pair_l=p(keep[3]),
                      q=0.05, c=0.0, std=1.0, origin=0.0, inv_mass=p(keep[4]))
    return m, keep


def _eval_empty(n_atoms):
    m, keep = _model(n_atoms)
    buf = _aligned(16)
    d = lambda: C.c_void_p(buf.ctypes.data)
    return lib.sc_gdml_eval_scratch(C.byref(m), C.c_void_p(keep[5].ctypes.data), d(), 0, d(), d(), d(), None)


@pytest.mark.parametrize("n_atoms", [49, 60, 128, 170])
def test_eval_accepts_molecules_up_to_170_atoms(n_atoms):
    assert _eval_empty(n_atoms) == SC_OK, lib.sc_last_error().decode()


def test_eval_refuses_171_atoms_and_names_the_limit():
    assert lib.sc_gdml_max_atoms() == 170
    assert _eval_empty(171) == SC_ERR_UNSUPPORTED
    assert "170" in lib.sc_last_error().decode()


def test_large_route_needs_its_scratch():
    m, keep = _model(60)
    buf = _aligned(16)
    d = lambda: C.c_void_p(buf.ctypes.data)
    assert lib.sc_gdml_eval(C.byref(m), d(), 0, d(), d(), d(), None) != SC_OK
    assert "scratch" in lib.sc_last_error().decode()


def test_scratch_bytes():
    for n in (2, 30, 48):
        assert lib.sc_gdml_scratch_bytes(n, 200) == 0
    for n, m in ((49, 200), (64, 200), (100, 17), (170, 200), (170, 5000)):
        b = lib.sc_gdml_scratch_bytes(n, m)
        # at least one geometry: XJ and AJ rows [M][3N] dominate
        assert b >= 8 * 2 * m * 3 * n and b % 8 == 0, (n, m, b)
    assert lib.sc_gdml_scratch_bytes(171, 200) < 0
    for name in ("sc_gdml_scratch_bytes", "sc_gdml_max_atoms", "sc_gdml_eval_scratch", "sc_gdml_stage_scratch"):
        assert name in SIGNATURES


def test_large_kernels_need_no_scratch_memory():
    """no private segment and no VGPR spills; the scalars kernel of the largest molecules spills SGPRs into VGPR lanes
    (no memory traffic; 72 at 29 descriptor elements per thread when measured)"""
    so = os.path.join(ROOT, "semiclassical_amd", "libsemiclassical_hip.so")
    assert os.path.exists(so), "build() first"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), so, "gdml_big"],
                         capture_output=True, text=True, check=True).stdout
    rows = [r for r in out.splitlines() if "gdml_big_" in r]
    assert len(rows) == 6, out
    for r in rows:
        scratch = re.search(r"scratch\s+(\d+) B", r)
        spills = re.search(r"spill v (\d+) s (\d+)", r)
        assert scratch and int(scratch.group(1)) == 0, r
        assert spills and spills.group(1) == "0" and int(spills.group(2)) <= 96, r
        if "scalars" not in r:
            assert spills.group(2) == "0", r
