"""The determinant tail off the item hand-over (csrc/sc_hk_step_sd.hip: the tail of item t runs inside phase B of item t + 1, the last
one of a workgroup in an epilogue) and the last diagonal block of the register elimination without its dead work (TRIM_LAST of
eliminate_block, csrc/sc_hk_lu.h).  Both change WHEN work happens, not what is computed: the bar is bits -- against the same inputs
run with one item per workgroup (only the epilogue path), against single steps, and against the parent commit's library
(tests/golden/lu_tail_parent_bits.npz, recorded by tools/record_lu_tail_parent_bits.py) -- plus the CPU oracle independently of
the fixture.  Inputs: the integer-hash dense states of tests/lu_trim_inputs.py, amplitude 0.3 for single steps and 1e-5 for visits
(tests/test_pair_no_mid_store_gpu.py: strictly row-diagonally dominant prefactor matrices, no weak pivot in any sub-step)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import lu_trim_inputs as inp
from tests import tail_offpath_inputs as tin
from tests import test_pair_no_mid_store_gpu as pairs
from tests import test_visit_steps_gpu as visits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lu_tail_parent_bits.npz")
# test_tails_*: the n = 3 grid + 5 trajectories repeat DISTINCT hash states (generating 354 MB of hash noise at D = 60 takes
# 15 s on the host).  The period is a prime that does not divide the grid, so the items a workgroup sees one after the other --
# tr, tr + grid, ... under the static hand-out, neighbours under the cursor -- never hold the same state: a tail that reads the
# buffers of the wrong parity or stores to the wrong trajectory shows.
DISTINCT = 251


def _many_items_state(D, amplitude):
    from semiclassical_amd._lib import lib
    grid = lib.sc_step_grid(10 ** 6, D)
    n = 3 * grid + 5
    assert grid % DISTINCT != 0
    _, y = inp.reference_state(D, DISTINCT, stream=5, amplitude=amplitude)
    return grid, n, np.ascontiguousarray(y[:, np.arange(n) % DISTINCT])


def _single(D, y):
    """prefactor-only launch, then one sc_hk_step: (c2, sgn, flags) after each and the blocks at the end, on the device"""
    prop, pot = inp.engine(D, y)
    n = y.shape[1]
    out = [torch.view_as_real(prop._c2).clone(), prop._sgn.clone(), prop._flags[:n + 1].clone()]
    prop.step(pot, inp.DT)
    torch.cuda.synchronize()
    out += [torch.view_as_real(prop._c2).clone(), prop._sgn.clone(), prop._flags[:n + 1].clone()]
    out.append(prop.y[2 * D:2 * D + 4 * D * D].t().contiguous())
    return out


@pytest.mark.parametrize("D", [17, 33, 60])
def test_tails_across_items_single_steps(D):
    """n = 3 grid + 5: every persistent workgroup has at least three items, so it runs deferred tails of both parities and the epilogue.
    Prefactor-only launch and one sc_hk_step at amplitude 0.3 (weak pivots and the fix-up launch included) against the same inputs
    in chunks of at most one grid, where every workgroup has one item and only the epilogue runs: c2, sgn, the per-trajectory
    flags and the flagged count of each chunk, and the blocks, bit for bit"""
    grid, n, y = _many_items_state(D, inp.NOISE)
    whole = _single(D, y)
    counts = [0, 0]
    for lo in range(0, n, grid):
        hi = min(n, lo + grid)
        part = _single(D, np.ascontiguousarray(y[:, lo:hi]))
        for k, (x, z) in enumerate(zip(whole, part)):
            if k in (2, 5):             # flags: per trajectory, and the count of the launch
                assert torch.equal(x[lo:hi], z[:hi - lo]), (lo, k)
                counts[k // 3] += int(z[hi - lo].item())
            else:
                assert torch.equal(x[lo:hi], z), (lo, k)
    print(D, "n", n, "grid", grid, "flagged (prefactor-only, step)", int(whole[2][n].item()), int(whole[5][n].item()), "chunks", counts)
    assert counts == [int(whole[2][n].item()), int(whole[5][n].item())]


@pytest.mark.parametrize("D,ks", [(17, 2), (33, 2), (33, 3), (60, 2), (60, 3)])
def test_tails_across_items_visits(D, ks):
    """the same for one visit of ks sub-steps (amplitude 1e-5, D = 17 has pairs only): the tails of a visit hand the determinant and
    sign on in LDS, the last one crosses to the next trajectory or to the epilogue.  State, blocks, c2, sgn and every intermediate
    (c2_mid, sgn_mid, q p, S) against chunks of at most one grid, bit for bit; no unrepaired intermediate determinant"""
    grid, n, y = _many_items_state(D, pairs.AMPLITUDE)
    assert pairs._row_dominance(D, y[:, :DISTINCT]) < 0.25
    a = visits._visit(D, y, ks)
    assert a._gstep == grid and int(a._multi["bad"].item()) == 0
    whole = visits._snapshot(a) + [a._mono.reshape(n, -1), a._flags[:n]] + [x.reshape(n, -1) for j in range(ks - 1) for x in visits._mid(a, j)]
    for lo in range(0, n, grid):
        hi = min(n, lo + grid)
        c = visits._visit(D, np.ascontiguousarray(y[:, lo:hi]), ks)
        assert int(c._multi["bad"].item()) == 0
        part = visits._snapshot(c) + [c._mono, c._flags[:hi - lo]] + [x for j in range(ks - 1) for x in visits._mid(c, j)]
        for k, (x, z) in enumerate(zip(whole, part)):
            assert torch.equal(x.reshape(n, -1)[lo:hi], z.reshape(hi - lo, -1)), (lo, k)


@pytest.fixture(scope="module")
def parent_bits():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def runs():
    """tail_offpath_inputs.run_paths(D), once per dimension"""
    return functools.lru_cache(maxsize=None)(tin.run_paths)


@pytest.mark.parametrize("D", tin.DIMS)
def test_every_shape_of_the_last_block_parent_bits(D, runs, parent_bits):
    """64 dense states per dimension, prefactor-only launch and three steps: c2, sgn, flagged counts and the blocks are those of the
    parent commit's library, bit for bit.  The amplitude is the fixture's (0.3 for every dimension: the parent's register elimination
    kept at least half of the trajectories everywhere, 28 of 64 flagged at the most), and it keeps half of them here too"""
    assert float(parent_bits[f"amplitude_{D}"][0]) == tin.AMPLITUDE[D]
    got = runs(D)
    for key, val in got.items():
        print(D, key, "equal" if np.array_equal(val, parent_bits[f"{key}_{D}"]) else "DIFFERENT")
    for key, val in got.items():
        assert np.array_equal(val, parent_bits[f"{key}_{D}"]), key
    assert 2 * int(parent_bits[f"pre_flagged_{D}"][0]) <= tin.NTRAJ and np.all(2 * parent_bits[f"step_flagged_{D}"] <= tin.NTRAJ)
    assert 2 * int(got["pre_flagged"][0]) <= tin.NTRAJ and np.all(2 * got["step_flagged"] <= tin.NTRAJ)


@pytest.mark.parametrize("D", tin.DIMS)
def test_every_shape_of_the_last_block_oracle(D, runs):
    """the same states: determinants of the prefactor-only launch against the CPU oracle's, 1e-10 relative"""
    _, y = inp.reference_state(D, tin.NTRAJ, amplitude=tin.AMPLITUDE[D])
    want = inp.oracle_c2(D, y)
    got = runs(D)["pre_c2"]
    err = np.max(np.abs(got - want) / np.abs(want))
    print(D, "max relative deviation from the oracle", err)
    assert err < 1e-10


def _crossed(a, b):
    """the branch rule (csrc/sc_common.h crossed_branch_cut) on arrays of determinants"""
    return (a.real < 0) & (b.real < 0) & (a.imag * b.imag < 0)


def test_tracker_through_deferred_tails():
    """a visit of three steps in which the determinant crosses the cut in sub-step 0 AND again in sub-step 1 of the same trajectory:
    the deferred tail of sub-step 1 must track against the determinant and the flipped sign that the tail of sub-step 0 left in
    LDS.  The determinant of a near-diagonal state turns by -sum(omega) dt per step, always the same way, so it cannot cross twice
    in a row; here dt = 24.8 makes that a full turn up to the anharmonic shifts (+-0.035 rad over the trajectories, +-0.01 from step
    to step), row 0 of every block is negated (c2(0) = -1 + O(1e-3) i), and the trajectories are chosen from the CPU oracle's
    determinants of the hash inputs (D = 33, stream 7, 512 states, amplitude 1e-5: six of them cross twice).  Against three single
    steps: signs, determinants and every intermediate, bit for bit; the chosen trajectories' signs are -1, +1 after sub-steps 0, 1"""
    from semiclassical_amd import _lib
    from oracle import sc_oracle as orc
    import bench
    D, n, dt = 33, 512, 24.8
    _, y = inp.reference_state(D, n, stream=7, amplitude=pairs.AMPLITUDE)
    for k in range(4):
        y[2 * D + k * D * D: 2 * D + k * D * D + D] *= -1.0
    assert pairs._row_dominance(D, y) < 0.25
    omega, chi, nac, q0, _ = bench.as60_model(D)
    G = torch.diag(omega)
    ref = orc.HKOracle(G, G)
    ref.set_initial_conditions(q0, 0.0 * q0, G, torch.from_numpy(y[:2 * D].copy()), torch.ones(n))
    ref.y = torch.from_numpy(y.copy())
    ref._prefactor()
    c = [ref.c2.numpy().copy()]
    for _ in range(2):
        ref.step(orc.MorseOracle(omega, chi, nac), dt)
        c.append(ref.c2.numpy().copy())
    twice = np.nonzero(_crossed(c[0], c[1]) & _crossed(c[1], c[2]))[0]
    print("trajectories that cross in sub-step 0 and again in sub-step 1:", twice.tolist())
    assert len(twice) >= 1
    a, pot = inp.engine(D, y)
    b, _ = inp.engine(D, y)
    a._launch_step_visit(a._potential_descriptor(pot, dt), dt, 3)
    torch.cuda.synchronize()
    assert int(a._multi["bad"].item()) == 0
    for j in range(3):
        b.step(pot, dt)
        torch.cuda.synchronize()
        got = visits._mid(a, j) if j < 2 else visits._snapshot(a)
        visits._assert_snapshot(got, visits._snapshot(b), f"after sub-step {j}")
        if j < 2:
            assert torch.all(got[2].cpu()[twice] == (-1.0 if j == 0 else 1.0))
    b._set_mono_layout(_lib.SC_MONO_TILED16)
    torch.cuda.synchronize()
    assert torch.equal(a._mono, b._mono)


@pytest.mark.parametrize("D,ks", [(48, 3), (60, 3)])
def test_weak_pivot_in_the_last_sub_step_last_item_and_not(D, ks):
    """the shifted blocks of tests/test_visit_steps_gpu.py (every leading pivot zero in every sub-step) on n = grid + 5 trajectories:
    five workgroups have two visits -- a weak last sub-step whose deferred tail runs inside the next trajectory's first item --
    and for all the others, and for those five's second visit, it is the workgroup's last item and runs in the epilogue.  The tail
    must restore c2 / sgn to the predecessor it kept in LDS, flag the trajectory and count it; the fix-up launch then gives the
    one-step path's state, blocks, determinants and flags.  (The branch sign is not compared: see
    test_weak_pivot_in_the_last_sub_step_finds_its_blocks there.)"""
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import lib
    grid = lib.sc_step_grid(10 ** 6, D)
    n = grid + 5
    y50 = visits._shifted_blocks(D, 50)
    y = np.ascontiguousarray(y50[:, np.arange(n) % 47])          # 47: prime, does not divide the grid
    assert grid % 47 != 0
    a = visits._visit(D, y, ks)
    assert a._gstep == grid
    b, pot = inp.engine(D, y)
    for _ in range(ks):
        b.step(pot, inp.DT)
    torch.cuda.synchronize()
    b._set_mono_layout(_lib.SC_MONO_TILED16)
    torch.cuda.synchronize()
    bad = int(a._multi["bad"].item())
    print(D, ks, "unrepaired", bad, "of", n, "flagged", inp.flagged(a), inp.flagged(b))
    for name in ("_qp", "_act", "_mono"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(torch.view_as_real(a._c2), torch.view_as_real(b._c2))
    assert torch.equal(a._flags[:n + 1], b._flags[:n + 1])
    assert bad == (ks - 1) * n
    with pytest.raises(_lib.EngineError):
        a.synchronize()
