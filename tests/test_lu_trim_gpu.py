"""The register elimination of the separable fast path (csrc/sc_hk_lu.h) after its trimming -- the last pivot step of a full
block peeled down to the trailing slots -- on DENSE blocks, so that the elimination really pivots (the benchmark's blocks are
diagonal).  The bar is the bits of the elimination before the change (tests/golden/lu_parent_bits.npz, recorded with the parent
commit's library by tools/record_lu_parent_bits.py from the same integer-hash inputs), plus the CPU oracle independently of that
fixture."""
import os

import numpy as np
import pytest
import torch

from tests import lu_trim_inputs as inp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lu_parent_bits.npz")


@pytest.fixture(scope="module")
def parent_bits():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def runs():
    """run_paths(D), once per dimension"""
    cache = {}

    def get(D):
        if D not in cache:
            cache[D] = inp.run_paths(D)
        return cache[D]
    return get


@pytest.mark.parametrize("D", inp.DIMS)
def test_bits_of_the_parent_elimination(D, runs, parent_bits):
    """prefactor-only launch and three sc_hk_step calls (AS model) on 64 dense states: c2, sgn, flagged counts and the blocks after
    the third step are those of the parent commit, bit for bit; the register path kept at least half of the trajectories"""
    got = runs(D)
    for key, val in got.items():
        want = parent_bits[f"{key}_{D}"]
        print(D, key, "equal" if np.array_equal(val, want) else "DIFFERENT")
    for key, val in got.items():
        assert np.array_equal(val, parent_bits[f"{key}_{D}"]), key
    assert 2 * int(got["pre_flagged"][0]) <= inp.NTRAJ
    assert np.all(2 * got["step_flagged"] <= inp.NTRAJ)


@pytest.mark.parametrize("D", inp.DIMS)
def test_dense_states_against_the_oracle(D, runs):
    """the same states: determinants of the prefactor-only launch against the CPU oracle's, 1e-10 relative"""
    _, y = inp.reference_state(D, inp.NTRAJ)
    want = inp.oracle_c2(D, y)
    got = runs(D)["pre_c2"]
    err = np.max(np.abs(got - want) / np.abs(want))
    print(D, "max relative deviation from the oracle", err)
    assert err < 1e-10


@pytest.mark.parametrize("D,row", [(60, 59), (17, 16)])
def test_zero_pivot_in_the_last_block(D, row):
    """a zero row in the LAST diagonal block of every second trajectory: c2 == 0 exactly there, the others as the oracle (1e-9)"""
    _, y = inp.reference_state(D, inp.NTRAJ, stream=3)
    for k in range(4):
        y[2 * D + k * D * D + row * D: 2 * D + k * D * D + (row + 1) * D, ::2] = 0.0
    prop, _ = inp.engine(D, y)
    got = prop._c2.cpu().numpy()
    want = inp.oracle_c2(D, y)
    assert np.all(got[::2] == 0.0)
    err = np.max(np.abs(got[1::2] - want[1::2]) / np.abs(want[1::2]))
    print(D, "max relative deviation of the regular trajectories", err)
    assert err < 1e-9


@pytest.mark.parametrize("D", [17, 33])
def test_buffer_parity_over_many_items_per_workgroup(D):
    """n = 3 * grid + 5: every persistent workgroup eliminates at least three trajectories (both parities of the double-buffered
    per-trajectory results, the resets in between).  Prefactor-only launch and one step, against the same inputs in chunks of at
    most one grid (every workgroup one trajectory), bit for bit."""
    from semiclassical_amd._lib import lib
    grid = lib.sc_step_grid(10 ** 6, D)
    n = 3 * grid + 5
    _, y = inp.reference_state(D, n, stream=5)
    prop, pot = inp.engine(D, y)
    assert prop._gstep == grid
    pre = prop._c2.cpu().numpy().copy()
    prop.step(pot, inp.DT)
    torch.cuda.synchronize()
    post, sgn = prop._c2.cpu().numpy().copy(), prop._sgn.cpu().numpy().copy()
    del prop
    for lo in range(0, n, grid):
        hi = min(n, lo + grid)
        part, pot = inp.engine(D, np.ascontiguousarray(y[:, lo:hi]))
        assert np.array_equal(part._c2.cpu().numpy(), pre[lo:hi])
        part.step(pot, inp.DT)
        torch.cuda.synchronize()
        assert np.array_equal(part._c2.cpu().numpy(), post[lo:hi]) and np.array_equal(part._sgn.cpu().numpy(), sgn[lo:hi])


def test_pairs_on_dense_blocks():
    """sc_hk_step_multi called directly on the dense D = 33 states: bit-identical to two sc_hk_step calls"""
    from semiclassical_amd import _lib
    D = 33
    _, y = inp.reference_state(D, inp.NTRAJ)
    a, pot = inp.engine(D, y)
    b, _ = inp.engine(D, y)
    desc = a._potential_descriptor(pot, inp.DT)
    a._launch_step_pair(desc, inp.DT)
    b.step(pot, inp.DT)
    b.step(pot, inp.DT)
    torch.cuda.synchronize()
    b._set_mono_layout(_lib.SC_MONO_TILED16)
    torch.cuda.synchronize()
    assert a._state.mono_layout == b._state.mono_layout
    for x, z in ((a._qp, b._qp), (a._act, b._act), (a._mono, b._mono), (a._sgn, b._sgn)):
        assert torch.equal(x, z)
    assert torch.equal(torch.view_as_real(a._c2), torch.view_as_real(b._c2))
