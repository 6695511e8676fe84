"""Direct tests of the two inversions behind the Walton-Manolopoulos prefactor (sc_wm_correlate: wm_small_kernel and its flagged
re-run, wm_kernel<false> on LDS, wm_kernel<true> on global scratch).

Seeded monodromy blocks of three families (tests/wm_cases.py: natural, momentum-heavy, far-pivot) are assigned to a propagator,
the WM kernel is launched once with track = 2 (signs +1: the branch tracker has its own suite) and every trajectory's detA, detM,
C_QQ, d-vector and correlation terms are compared with the same terms in numpy.clongdouble:

    err <= 16 err64 + 4 m 2^-52,

err64 being the error of the fp64 oracle (WMOracle: torch / LAPACK) for that trajectory and quantity against the same reference, m
the order of the matrix behind the quantity, errors relative to the largest magnitude of the quantity.  The shapes are the smallest
at which the kernels change: one and several pivot candidates per lane (E = 2 d' up to and beyond 64), one and several columns of
the augmented matrix per thread (4 d' up to and beyond 256).  Before the pivot search covered the whole column and the row update
every column, d' >= 65 failed in every family (columns from 256 on were never eliminated) and far-pivot failed wherever a
dominant entry lies 64 or more rows below the diagonal."""
import numpy as np
import pytest
import torch

from tests import wm_cases as wc
from tests.det_cases import CLD

pytestmark = pytest.mark.gpu


def _launch(c):
    """-> propagator after one WM launch (track = 2) on the state of case c, with the coupling vectors of its constant potential"""
    from semiclassical_amd import propagators as PR
    torch.set_default_dtype(torch.float64)
    T = lambda x: torch.from_numpy(np.array(x))
    y, zi = wc.reference_state(c)
    prop = PR.WaltonManolopoulosPropagator(T(c.Gi), T(c.Gt), c.alpha, c.beta, device="cuda")
    prop.set_initial_conditions(T(c.q0), T(c.p0), T(c.G0), T(zi), T(c.probi))
    assert prop._wm_host.dprime == c.dp and prop._ntraj_norm == c.n
    prop.y = T(y)
    prop._remember_nac(wc.ConstantCoupling(c.tau1, c.tau2))
    prop._wm_launch(2)
    prop.synchronize()
    return prop


@pytest.mark.parametrize("family", wc.FAMILIES)
@pytest.mark.parametrize("D,dp", wc.SHAPES, ids=[f"{D}-{dp}" for D, dp in wc.SHAPES])
def test_wm_terms_match_the_extended_reference(D, dp, family):
    from semiclassical_amd._lib import lib
    c = wc.inputs(D, dp, family)
    ref = wc.reference(D, dp, family)
    prop = _launch(c)
    cnp = lambda t: t.detach().cpu().numpy()
    assert (lib.sc_wm_scratch_bytes(c.n, D, dp) > 0) == (prop._wm_scratch is not None)
    assert np.all(cnp(prop._sgnA) == 1.0) and np.all(cnp(prop._sgnM) == 1.0)           # track = 2
    got = {"detA": cnp(prop._detA), "detM": cnp(prop._detM), "cq": cnp(prop._cq), "kq": cnp(prop._kq)}
    chk = np.sqrt(cnp(prop._c2).astype(CLD)) * cnp(prop._sgn).astype(CLD)            # the HK factor the kernel read: an input
    _, cqq, dvec = prop._export()
    prop.synchronize()
    got["CQQ"], got["dvec"] = cnp(cqq), cnp(dvec)
    worst = {}
    failures = []
    for t in range(c.n):
        for qn in wc.QUANTITIES:
            want = ref[t][qn] * chk[t] if qn in ("cq", "kq") else ref[t][qn]
            e64, bound = wc.err64(D, dp, family, t, qn), wc.accuracy_bound(D, dp, family, t, qn)
            err = wc.rel_err(got[qn][t], want) if np.all(np.isfinite(got[qn][t])) else np.inf
            w = worst.setdefault(qn, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], err), max(w[1], e64), max(w[2], err / bound)
            if not err <= bound:
                failures.append((t, qn, err, e64, bound))
    flagged = int(prop._wm_flags[-1].item())
    print(f"WMSTAT D={D} d'={dp} family={family} flagged={flagged}/{c.n} "
          + " ".join(f"{qn}: err={w[0]:.1e} err64={w[1]:.1e} err/bound={w[2]:.2g}" for qn, w in worst.items()))
    assert not failures, (D, dp, family, failures)
