"""Premises of tests/test_branch_tracking_gpu.py, checked with the oracle alone: every row really contains flips in both
directions of Im, predecessors that must not flip, determinants with a margin from the axes, and -- for the two-step rows --
the flips the engine has to get right.  A broken construction fails here, without a GPU."""
import mpmath
import numpy as np
import pytest
import torch

from tests import branch_cases as B

torch.set_default_dtype(torch.float64)


@pytest.mark.parametrize("name,route,make_case,make_blocks,n,kw", B.ONE_STEP, ids=[r[0] for r in B.ONE_STEP])
def test_one_step_premise(name, route, make_case, make_blocks, n, kw):
    case, ref, y, setup = B.one_step_setup(make_case, make_blocks, n, **kw)
    assert set(setup) == set(B.keys_of(ref))
    want = B.oracle_step_from(ref, ref.y, setup, case.oracle_pot, case.dt)
    for key, (z, prev, sgn, cat) in setup.items():
        # the oracle's tracker flipped exactly the FLIP category
        flipped = want.tracker.signs(key).real != sgn
        assert torch.equal(flipped, cat == B.FLIP), key
        assert torch.allclose(want.tracker.state[key]["previous"], z, rtol=0, atol=0), key


@pytest.mark.parametrize("name,make_case,nt,normal_modes", B.WHOLE_LOOP, ids=[r[0] for r in B.WHOLE_LOOP])
def test_whole_loop_premise(name, make_case, nt, normal_modes):
    case, ref, y, setup = B.one_step_setup(make_case, B.dense_blocks, 256, seed=2)
    z, prev, sgn, cat = setup["prefactorC"]
    assert int((cat == B.FLIP).sum()) >= B.MIN_PER_CATEGORY


@pytest.mark.parametrize("D", [33, 60])
def test_two_step_pair_premise(D):
    case, n, seed = B.morse_case(D), 256, 1
    ref = case.oracle(n, seed)
    y = B.with_blocks(ref.y, D, B.dense_blocks(D, n, torch.Generator().manual_seed(seed), torch.diagonal(case.Gi),
                                                noise=B.PAIR_NOISE))
    z1, z2, prev, sgn, f1, f2 = B.pair_setup(ref, y, case.oracle_pot, case.dt, seed)
    counts = B.pair_counts(f1, f2)
    assert min(counts.values()) >= B.MIN_PER_CATEGORY, counts
    want = B.oracle_step_from(ref, y, {"prefactorC": (None, prev, sgn, None)}, case.oracle_pot, case.dt, steps=2)
    assert torch.equal(want.tracker.signs("prefactorC").real, sgn * torch.where(f1 ^ f2, -1.0, 1.0))


def _det_mp(mat):
    """determinant at 30 significant digits (mpmath LU)"""
    with mpmath.workdps(30):
        m = mpmath.matrix([[mpmath.mpc(complex(x)) for x in row] for row in mat.tolist()])
        return complex(mpmath.det(m))


def test_weak_last_sub_step_premise():
    """the weak-last-sub-step construction: entry (i, i) of the prefactor matrix vanishes after the second step only, the
    intermediate step flips for some trajectories, and tracking the final determinant against the value from before the pair
    (the wrong predecessor) gives other signs than the oracle.  The near-singular determinants are checked at 30 digits."""
    D, row, col, n, seed, make_case = B.WEAK_LAST
    case = make_case()
    ref = case.oracle(n, seed)
    y = B.with_blocks(ref.y, D, B.weak_last_blocks(ref, case.oracle_pot, case.dt, row, col, seed + 3))
    first, second = B.weak_last_premise(ref, y, case.oracle_pot, case.dt, row, col)
    assert float(first.min()) > 0.25 and float(second.max()) < 1e-9
    z1, z2, prev, sgn, f1, f2 = B.pair_setup(ref, y, case.oracle_pot, case.dt, seed + 3)
    assert int(f1.sum()) >= B.MIN_PER_CATEGORY
    assert int((B.would_flip(prev, z2) != (f1 ^ f2)).sum()) >= B.MIN_PER_CATEGORY
    # torch.det of the near-singular prefactor matrices against a 30-digit elimination
    r = B.oracle_from(ref, y)
    for z in (z1, z2):
        r.step(case.oracle_pot, case.dt)
        mats = B.prefactor_matrix(r)
        for t in range(0, n, 8):
            exact = _det_mp(mats[t].numpy())
            assert abs(complex(z[t]) - exact) < 1e-11 * abs(exact), t
            assert np.sign(exact.real) == np.sign(float(z[t].real)) and np.sign(exact.imag) == np.sign(float(z[t].imag))
