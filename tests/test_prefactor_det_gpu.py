"""Direct tests of the complex determinant behind the HK prefactor, on every route sc_dense_mono_step(mode = 1) takes it:

  R  dense_prefactor_reg_kernel<NR> (block-pivoted register elimination) + fix-up of flagged trajectories by the LDS kernel
  L  dense_prefactor_kernel -> lds_lu_det on LDS
  G  prefactor_any_kernel -> lds_lu_det on a per-workgroup block of global scratch (D > 96)

Chosen complex matrices are encoded exactly into monodromy blocks (tests/det_cases.py) and the c2 the kernels return is compared
per matrix with an LU in numpy.clongdouble: err <= 16 err64 + 4 d 2^-52, err64 being LAPACK's fp64 error against the same
reference for the same matrix.  The matrices include the pivot-hostile ones no dynamics produces: cyclic shifts with exact zeros
whose column-0 pivot sits in row 63 ... 129 or d - 1 (beyond the 128 rows lds_lu_det used to search: c2 = 0 for a regular
matrix at d >= 129 before the search covered the whole column), the same with noise, permutation matrices of both parities, and
singular matrices."""
import numpy as np
import pytest
import torch

from tests import det_cases as dc

pytestmark = pytest.mark.gpu

DIAG_CASES = ([("R", D) for D in dc.ROUTE_R_DIMS] + [("L", D) for D in dc.ROUTE_L_DIMS] + [("G", D) for D in dc.ROUTE_G_DIMS])
SELECT_CASES = [("L", D, dp) for D, dp in dc.ROUTE_L_SELECT] + [("G", D, dp) for D, dp in dc.ROUTE_G_SELECT]


def _crosses_block(perm):
    """a monomial matrix (A[i, perm[i]] != 0, exact zeros elsewhere) has an entry outside the diagonal 16 x 16 blocks: the
    register elimination pivots inside those blocks only, meets an exact zero there, and must hand the trajectory on"""
    i = np.arange(len(perm))
    return bool(np.any(i // 16 != np.asarray(perm) // 16))


def _expected_flags(family, d, m, n):
    """(lower, upper) bound on the flagged count of each batch of n out of the m matrices of a family, or None"""
    if family == "generic":
        return [(0, 0)] * (m // n)
    if family == "gaussian":                          # no dominant diagonal: a weak in-block pivot may or may not occur
        return [(0, n)] * (m // n)
    if family == "shift":
        rows = dc.pivot_rows(d)
        hit = [_crosses_block(dc.shift_parts(d, rows[i % len(rows)])[0]) for i in range(m)]
    elif family == "permutation":
        hit = [_crosses_block(dc.permutation_parts(d, i % 2)[0]) for i in range(m)]
    elif family == "shift_noise":
        # large entries in a later column block than their row's: weak in-block pivots, for every shift once there are two blocks
        return [(1, n) if d > 16 else (0, 0)] * (m // n)
    else:                                             # singular: the matrices with a zero row meet an exact-zero pivot (bit 1 of weak)
        k = 3 if d >= 2 else 2
        hit = [i % k == k - 1 for i in range(m)]
        return [(sum(hit[b:b + n]), n) for b in range(0, m, n)]
    return [(sum(hit[b:b + n]),) * 2 for b in range(0, m, n)]


def _check_family(route, family, d, variant=None, select_D=None, twice=False):
    n = dc.batch_size(d if select_D is None else select_D)
    case = dc.family_cases(family, d, n)
    if case is None:
        return                                         # no shift / permutation at d = 1
    A, ref = case
    m = A.shape[0]
    got, flagged = np.empty(m, dtype=np.complex128), []
    for b in range(0, m, n):
        c2, sgn, fl = dc.run_route(route, A[b:b + n], variant or "plain", select_D)
        assert np.all(sgn == 1.0), (route, family, d, b)                 # mode 1 sets the branch sign
        got[b:b + n] = c2
        flagged.append(fl)
        if twice:
            again, _, _ = dc.run_route(route, A[b:b + n].copy(), variant or "plain", select_D)
            assert torch.equal(torch.from_numpy(c2.view(np.float64)), torch.from_numpy(again.view(np.float64))), \
                (route, family, d, b, c2, again)
    tag = f"DETSTAT route={route} family={family} D={select_D or d} d={d} widths={'select' if select_D else variant}"
    if route == "R":
        for b, (fl, (lo, hi)) in enumerate(zip(flagged, _expected_flags(family, d, m, n))):
            assert lo <= fl <= hi, (family, d, b, fl, lo, hi)
    assert np.all(np.isfinite(got.view(np.float64))), (route, family, d, got)
    if family == "singular":
        bound = 1e-12 * np.prod(np.linalg.norm(A, axis=2), axis=1)
        print(f"{tag} max|c2|/prod|row|={np.max(np.abs(got) / np.maximum(bound * 1e12, 1e-300)):.2e} flagged={flagged}")
        assert np.all(np.abs(got) <= bound), (route, d, np.abs(got), bound)
        return
    err, e64, bound = dc.rel_err(got, ref), dc.err64(A, ref), dc.accuracy_bound(A, ref)
    ratio = float(np.max(err / np.maximum(e64, 2.0 ** -53)))
    print(f"{tag} err={err.max():.2e} err64={e64.max():.2e} err/err64={ratio:.2f} err/bound={np.max(err / bound):.3f} flagged={flagged}")
    if family == "permutation":
        q = (got.astype(dc.CLD) / ref).astype(np.complex128)
        assert np.all(q.real > 0.0), (route, d, q)                                   # the sign of every exchange is kept
        assert np.all(np.abs(np.angle(q)) <= 1e-13), (route, d, np.angle(q))
    assert np.all(err <= bound), (route, family, d, variant, select_D, err, bound)


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("route,D", DIAG_CASES, ids=[f"{r}{D}" for r, D in DIAG_CASES])
def test_determinant_diagonal_widths(route, D, family):
    """st = si = 1 (A = Mqq / 2 + i Mpq / 2) and per-index power-of-two widths with all four blocks in play"""
    for variant in ("plain", "scaled"):
        _check_family(route, family, D, variant=variant, twice=(route == "G" and variant == "plain"))


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("route,D,dp", SELECT_CASES, ids=[f"{r}{D}-{dp}" for r, D, dp in SELECT_CASES])
def test_determinant_selected_submatrix(route, D, dp, family):
    """dense widths whose L, R select d' rows and d' other columns: general_prefactor_matrix_t<1>, <3>, its panelised form at
    (96, 96), and the X1 / X2 path of prefactor_any_kernel"""
    _check_family(route, family, dp, select_D=D, twice=(route == "G"))


def test_route_G_reuses_a_workgroups_scratch_beyond_256_trajectories():
    """the grid of prefactor_any_kernel is capped at 256 workgroups: with n = 259 three of them take a second trajectory and
    form its matrix in the scratch block the first one was eliminated in"""
    D, n = 97, 259
    base, base_ref = dc.family_cases("generic", D, dc.batch_size(D))
    more, more_ref = dc.family_cases("shift_noise", D, dc.batch_size(D))
    pool, pool_ref = np.concatenate((base, more)), np.concatenate((base_ref, more_ref))
    idx = np.arange(n) % len(pool)
    assert len(pool) % 256 != 0 and idx[256] != idx[0]
    A, ref = pool[idx], pool_ref[idx]
    c2, sgn, _ = dc.run_route("G", A)
    again, _, _ = dc.run_route("G", A.copy())
    assert np.all(sgn == 1.0)
    assert torch.equal(torch.from_numpy(c2.view(np.float64)), torch.from_numpy(again.view(np.float64)))
    err, bound = dc.rel_err(c2, ref), dc.accuracy_bound(pool, pool_ref)[idx]
    print(f"DETSTAT route=G n=259 D=97 err={err.max():.2e} err/bound={np.max(err / bound):.3f} last three {err[256:]}")
    assert np.all(err <= bound), (err, bound)
