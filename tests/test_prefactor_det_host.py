"""Host side of the direct determinant tests: the extended-precision reference, the exact encodings and the matrix families
of tests/det_cases.py have to satisfy on their own the conditions the GPU tests (test_prefactor_det_gpu.py) lean on."""
import numpy as np
import pytest

from tests import det_cases as dc


def test_long_double_is_extended_precision():
    """a platform where long double is double must fail loudly: the reference would be no better than the kernels"""
    assert np.finfo(np.longdouble).eps < 1.1e-19
    assert np.finfo(np.clongdouble).eps < 1.1e-19


def _mpf(x):
    """a long double as an mpmath number without loss: its double part plus the remainder"""
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - np.longdouble(hi)))


def test_det_longdouble_matches_mpmath():
    import mpmath
    d = 12
    with mpmath.workdps(50):
        for a in dc.generic(d, 3):
            want = mpmath.det(mpmath.matrix([[mpmath.mpc(complex(x)) for x in row] for row in a]))
            got = dc.det_longdouble(a)
            err = abs(mpmath.mpc(_mpf(got.real), _mpf(got.imag)) - want) / abs(want)
            assert err < 100 * d * 1.1e-19, float(err)


def test_det_longdouble_matches_analytic_permutations():
    d = 300
    for odd in (0, 1):
        perm, ph = dc.permutation_parts(d, odd)
        assert dc.permutation_sign(perm) == (-1 if odd else 1)
        want = dc.monomial_det(perm, ph)
        got = dc.det_longdouble(dc.permutation(d, odd))
        assert abs(got - want) / abs(want) < d * 1.1e-19
    assert dc.permutation_sign([1, 0, 2]) == -1 and dc.permutation_sign([1, 2, 0]) == 1 and dc.permutation_sign([0]) == 1


def test_det_longdouble_matches_analytic_shifts_beyond_the_old_search_window():
    d = 168
    for row in (63, 128, 138, d - 1):
        want = dc.monomial_det(*dc.shift_parts(d, row))
        assert abs(dc.det_longdouble(dc.shift(d, row)) - want) / abs(want) < d * 1.1e-19


@pytest.mark.parametrize("variant", ["plain", "scaled"])
@pytest.mark.parametrize("D", [1, 2, 17, 96, 130])
def test_diagonal_encoding_is_exact(D, variant):
    A = dc.generic(D, 3)
    st, si = dc.width_scales(D, variant)
    if variant == "scaled" and D > 2:
        assert len(set(st)) > 1 and len(set(si)) > 1 and not np.array_equal(st, si)
    M = dc.blocks_for(A, variant)
    assert M.shape == (3, 4, D, D)
    assert np.array_equal(dc.prefactor_diag_numpy(M, st, si), A)
    if variant == "scaled" and D > 2:            # the encoding tells st from si and rows from columns
        assert not np.array_equal(dc.prefactor_diag_numpy(M, si, st), A)
        assert not np.array_equal(dc.prefactor_diag_numpy(M.swapaxes(-1, -2), st, si), A.swapaxes(-1, -2))


@pytest.mark.parametrize("D,dp", dc.ROUTE_L_SELECT + dc.ROUTE_G_SELECT[:4])
def test_selection_encoding_is_exact(D, dp):
    A = dc.generic(dp, 2)
    rows, cols, L, R = dc.selection(D, dp)
    assert len(set(rows)) == dp and len(set(cols)) == dp
    assert np.array_equal(L.imag, 0 * L.imag) and np.array_equal(R.imag, 0 * R.imag)
    assert np.array_equal(L.real.sum(axis=1), np.ones(dp)) and np.array_equal(R.real.sum(axis=0), np.ones(dp))
    big = dc.embed(A, D)
    assert np.array_equal(big[:, rows][:, :, cols], A)
    if D > dp:
        assert not np.array_equal(big[:, :dp, :dp], A)
    M = dc.blocks_for(big, "plain")
    assert np.array_equal(dc.prefactor_general_numpy(M, L, L, R, R), A)


def test_pivot_rows_straddle_the_search_windows():
    assert dc.pivot_rows(1) == () and dc.pivot_rows(2) == (1,)
    assert dc.pivot_rows(64) == (63,) and dc.pivot_rows(65) == (63, 64)
    assert dc.pivot_rows(129) == (63, 64, 65, 127, 128)
    assert dc.pivot_rows(168) == (63, 64, 65, 127, 128, 129, 167)
    for d in (2, 65, 130, 300):
        for r in dc.pivot_rows(d):
            a = dc.shift(d, r)
            assert np.flatnonzero(a[:, 0]).tolist() == [r]


@pytest.mark.parametrize("d", dc.all_dims())
def test_families_meet_what_the_gpu_tests_assume(d):
    """|det| stays inside 1e-100 ... 1e100 (neither the kernels nor the reference protect the running product), and LAPACK in
    fp64 is within 1e-12 of the reference: the GPU bound 16 err64 + 4 d 2^-52 is then tight for every case"""
    n = dc.batch_size(d)
    for family in dc.FAMILIES:
        case = dc.family_cases(family, d, n)
        if case is None:
            assert d < 2 and family != "generic" and family != "singular"
            continue
        A, ref = case
        assert A.shape[0] % n == 0 and A.shape[1:] == (d, d) and A.dtype == np.complex128
        norms = np.prod(np.linalg.norm(A, axis=2).astype(np.longdouble), axis=1)
        if family == "singular":
            assert ref is None
            live = norms > 0                     # a zero row makes the bound itself zero: the determinant is exactly 0
            assert np.all(np.abs(np.linalg.det(A)[live]) <= 1e-12 * norms[live].astype(np.float64))
            assert np.all((norms[live] > 1e-100) & (norms[live] < 1e100))
            continue
        mag = np.abs(ref)
        assert np.all((mag > 1e-100) & (mag < 1e100)), (family, float(mag.min()), float(mag.max()))
        e = dc.err64(A, ref)
        assert e.max() < 1e-12, (family, e.max())
        assert np.all(dc.accuracy_bound(A, ref) < 1e-11)
