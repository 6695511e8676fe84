"""Host side of the direct Walton-Manolopoulos tests (tests/wm_cases.py, tests/test_wm_inverse_gpu.py): the extended-precision
reference against the fp64 oracle on every shape and family, finiteness and the conditioning cap of the inputs, the elimination
helper on matrices with known inverse and determinant, and the sharpness of the far-pivot family: a plain fp64 Gauss-Jordan whose
pivot search stops 64 rows below the diagonal has to break the bound of the GPU test, the same elimination with the whole column
in view has to keep it."""
import numpy as np
import pytest

from tests import det_cases as dc
from tests import wm_cases as wc

CASES = [(D, dp, f) for D, dp in wc.SHAPES for f in wc.FAMILIES]
IDS = [f"{D}-{dp}-{f}" for D, dp, f in CASES]
FAR = [(D, dp) for D, dp in wc.SHAPES if dp > wc.WINDOW]
NEAR = [(D, dp) for D, dp in wc.SHAPES if dp <= wc.WINDOW]
TINY, HUGE = 1e-290, 1e290


def _c128(x):
    return np.asarray(x, dtype=np.complex128)


def test_gauss_jordan_on_known_matrices():
    """inverse and determinant of the elimination helper, full and windowed search, fp64 and extended"""
    for d, row in ((5, 3), (66, 65), (130, 64)):
        perm, fac = dc.shift_parts(d, row)
        A = dc.shift(d, row)
        for ct in (np.complex128, dc.CLD):
            inv, det = wc.gauss_jordan(A.astype(ct))
            want = dc.monomial_det(perm, fac)
            assert abs(complex(det / want - 1.0)) < 1e-13 and inv.dtype == ct
            assert np.max(np.abs(_c128(inv @ A.astype(ct) - np.eye(d)))) < 1e-14
            assert abs(complex(dc.det_longdouble(A) / want - 1.0)) < 1e-16
        # the only entry of column 0 sits in row `row`: a search of 64 rows misses it from row 64 on
        _, det = wc.gauss_jordan(A, window=wc.WINDOW)
        assert (det == 0) == (row >= wc.WINDOW)
    rng = np.random.default_rng(3)
    A = rng.standard_normal((40, 40)) + 1j * rng.standard_normal((40, 40))
    inv, det = wc.gauss_jordan(A.astype(dc.CLD))
    assert np.max(np.abs(_c128(inv @ A.astype(dc.CLD) - np.eye(40)))) < 1e-15
    assert abs(complex(det / dc.det_longdouble(A) - 1.0)) < 1e-15
    assert wc.rel_err(np.linalg.inv(A), inv) < 1e-12


@pytest.mark.parametrize("D,dp,family", CASES, ids=IDS)
def test_inputs_are_finite_and_well_conditioned(D, dp, family):
    """nothing overflows or underflows in the oracle or in the reference, and the fp64 oracle is within 1e-9 of the reference for
    every trajectory and quantity the GPU test uses (1e-12 in the natural family: the Filinov matrix of symplectic blocks of
    order 1 has a condition number of a few tens, E = 258 elimination steps at most)"""
    c, ref, orc = wc.inputs(D, dp, family), wc.reference(D, dp, family), wc.oracle_terms(D, dp, family)
    assert c.n in range(4, 9)
    for name in ("Gi", "Gt", "G0", "iGi0", "iG0", "U", "blocks", "q", "p", "Q", "P", "S", "probi", "n1"):
        assert np.all(np.isfinite(getattr(c, name))), name
    assert all(TINY < abs(x) < HUGE for x in c.dets)
    cap = 1e-12 if family == "natural" else wc.ERR64_CAP
    for t in range(c.n):
        for qn in wc.QUANTITIES:
            for val in (_c128(ref[t][qn]), _c128(orc[t][qn])):
                assert np.all(np.isfinite(val)) and TINY < np.max(np.abs(val)) < HUGE, (t, qn)
            e = wc.err64(D, dp, family, t, qn)
            assert e < cap, (D, dp, family, t, qn, e)


@pytest.mark.parametrize("D,dp", wc.SHAPES, ids=[f"{D}-{dp}" for D, dp in wc.SHAPES])
def test_momentum_heavy_blocks_make_the_elimination_permute(D, dp):
    """in the momentum-heavy family the imaginary part of A'/s outweighs its real part and the diagonal does not dominate: the
    largest entry of most columns is off the diagonal"""
    ref = wc.reference(D, dp, "momentum-heavy")
    As = _c128(ref[0]["As"])
    assert np.linalg.norm(As.imag) > 2.0 * np.linalg.norm(As.real)
    off = np.argmax(np.abs(As), axis=0) != np.arange(2 * dp)
    assert np.count_nonzero(off) > dp, np.count_nonzero(off)


def _emulated(c, t, window):
    return wc.wm_terms(c, t, 1.0, ct=np.complex128, inverse=lambda A: wc.gauss_jordan(A, window), det=None)


@pytest.mark.parametrize("D,dp", FAR, ids=[f"{D}-{dp}" for D, dp in FAR])
def test_far_pivot_family_is_sharp(D, dp):
    """d' >= 65.  The family's entries lie 64 or more rows below the diagonal and exceed everything within 64 rows of their
    column by 2^20 or more, in A'/s and (through C_QQ) in M'/2 pi; the windowed fp64 elimination violates the bound for every
    trajectory, the full search keeps it for every trajectory and quantity."""
    c, ref = wc.inputs(D, dp, "far-pivot"), wc.reference(D, dp, "far-pivot")
    entries = wc.far_pivot_entries(dp)
    assert len(entries) == min(4, dp - wc.WINDOW) and (dp <= 2 * wc.WINDOW or (2 * wc.WINDOW, 0) in entries)
    for t in range(c.n):
        As, Ms = _c128(ref[t]["As"]), _c128(ref[t]["Ms"])
        for r, k in entries:
            assert r - k >= wc.WINDOW
            assert np.abs(As[r, k]) >= wc.FAR_FACTOR * np.max(np.abs(As[k:r, k])), (t, r, k)
            assert np.argmax(np.abs(Ms[k:, k])) + k == r and np.abs(Ms[r, k]) > 2.0 ** 10 * np.max(np.abs(Ms[k:r, k]))
        full, win = _emulated(c, t, None), _emulated(c, t, wc.WINDOW)
        broken = []
        for qn in wc.QUANTITIES:
            bound = wc.accuracy_bound(D, dp, "far-pivot", t, qn)
            assert wc.rel_err(full[qn], ref[t][qn]) <= bound, (t, qn)
            if not wc.rel_err(win[qn], ref[t][qn]) <= bound:
                broken.append(qn)
        assert {"detA", "detM", "cq", "kq"} <= set(broken), (t, broken)
        if dp > 2 * wc.WINDOW:
            # the entry of column 0 in row 128 is beyond a search of 128 rows as well (two candidates per lane and no more)
            win = _emulated(c, t, 2 * wc.WINDOW)
            broken = [qn for qn in wc.QUANTITIES if not wc.rel_err(win[qn], ref[t][qn]) <= wc.accuracy_bound(D, dp, "far-pivot", t, qn)]
            assert {"detA", "detM", "cq", "kq"} <= set(broken), (t, broken)


@pytest.mark.parametrize("D,dp", NEAR, ids=[f"{D}-{dp}" for D, dp in NEAR])
def test_far_pivot_family_below_65_dimensions(D, dp):
    """d' <= 64: the same drift and kick with the pairs the order allows.  The full fp64 elimination keeps the bound.  For
    E = 2 d' >= 66 the entries c B K of the lower left block sit 64 rows below the diagonal (far_pivot_entries), but the kick c K
    itself is symmetric and puts an entry c within 64 rows of the same column, so a windowed search is not led astray here
    (DESIGN.md section 4.4 says why no well-conditioned case does that below d' = 65)."""
    c, ref = wc.inputs(D, dp, "far-pivot"), wc.reference(D, dp, "far-pivot")
    if 2 * dp > wc.WINDOW:
        for t in range(c.n):
            As = _c128(ref[t]["As"])
            for r, k in wc.far_pivot_entries(dp):
                assert r - k >= wc.WINDOW and np.abs(As[r, k]) >= wc.NEAR_FACTOR * np.abs(As[k, k]), (t, r, k)
    for t in range(c.n):
        full = _emulated(c, t, None)
        for qn in wc.QUANTITIES:
            assert wc.rel_err(full[qn], ref[t][qn]) <= wc.accuracy_bound(D, dp, "far-pivot", t, qn), (t, qn)
