"""Up to four time steps per visit of a trajectory (sc_hk_step_visit, include/semiclassical_hip.h): sub-step ks of a visit loads the
blocks of the visit's start, applies the row propagators P(0) .. P(ks) one after the other and eliminates; only the last sub-step
stores.  The bar is bit-identity with ksteps launches of the one-step kernel, on the DENSE states of tests/lu_trim_inputs.py (a
wrong or misplaced row propagator is invisible on diagonal blocks), with the off-diagonal amplitude of
tests/test_pair_no_mid_store_gpu.py (no weak pivot in any intermediate determinant: reasoning there).  run() itself takes visits on
diagonal blocks only; its tail (nt mod visit_steps) and its launch sequence are checked on the AS model."""
import functools

import numpy as np
import pytest
import torch

from tests import lu_trim_inputs as inp
from tests import test_pair_no_mid_store_gpu as pairs

pytestmark = pytest.mark.gpu

AMPLITUDE = pairs.AMPLITUDE
STATE = ("_qp", "_act", "_sgn")


def _snapshot(prop):
    """(q p, S, sign, determinant) of the current state"""
    return [getattr(prop, name).clone() for name in STATE] + [torch.view_as_real(prop._c2).clone()]


@functools.lru_cache(maxsize=None)
def _single_steps(D, n=inp.NTRAJ, stream=0, nsteps=4):
    """the dense state of dimension D advanced by one sc_hk_step launch at a time: snapshots after every step and the blocks in the
    tiled layout after steps 3 and 4 (computed once per D, read by the KS = 3 and the KS = 4 case, never written)"""
    from semiclassical_amd import _lib
    _, y = inp.reference_state(D, n, stream=stream, amplitude=AMPLITUDE)
    assert pairs._row_dominance(D, y) < 0.25
    b, pot = inp.engine(D, y)
    snaps, mono = [], {}
    for k in range(1, nsteps + 1):
        b.step(pot, inp.DT)
        torch.cuda.synchronize()
        snaps.append(_snapshot(b))
        if k >= 3:
            b._set_mono_layout(_lib.SC_MONO_TILED16)
            torch.cuda.synchronize()
            mono[k] = b._mono.clone()
    return y, snaps, mono


def _visit(D, y, ks):
    from semiclassical_amd import _lib
    a, pot = inp.engine(D, y)
    a._launch_step_visit(a._potential_descriptor(pot, inp.DT), inp.DT, ks)
    torch.cuda.synchronize()
    assert a._state.mono_layout == _lib.SC_MONO_TILED16
    return a


def _mid(a, j):
    """the j-th intermediate state of the last visit as _snapshot() gives it"""
    m, n = a._multi, a.ntraj
    rows = slice(j * n, (j + 1) * n)
    return [m["qp"][rows].reshape(a._qp.shape), m["act"][rows], m["sgn"][rows], torch.view_as_real(m["c2"][rows])]


def _assert_snapshot(got, want, what):
    for name, x, z in zip(STATE + ("_c2",), got, want):
        same = torch.equal(x.reshape(-1), z.reshape(-1))
        print(what, name, "equal" if same else f"DIFFERENT in {int((x.reshape(-1) != z.reshape(-1)).sum())} of {x.numel()} elements")
    for name, x, z in zip(STATE + ("_c2",), got, want):
        assert torch.equal(x.reshape(-1), z.reshape(-1)), (what, name)


@pytest.mark.parametrize("D", [33, 48, 60, 64])
@pytest.mark.parametrize("ks", [3, 4])
def test_visit_equals_single_steps_on_dense_blocks(D, ks):
    """one visit of ks sub-steps against ks sc_hk_step launches: the final state, action, blocks (tiled), signs and determinants, and
    every intermediate (q p, S, sign, determinant), bit for bit.  NR = 3: D = 33 (one row in the last tile), 48 (full); NR = 4: 60, 64"""
    y, snaps, mono = _single_steps(D)
    a = _visit(D, y, ks)
    assert int(a._multi["bad"].item()) == 0
    for j in range(ks - 1):
        _assert_snapshot(_mid(a, j), snaps[j], f"D={D} ks={ks} after sub-step {j}")
    _assert_snapshot(_snapshot(a), snaps[ks - 1], f"D={D} ks={ks} final")
    assert torch.equal(a._mono, mono[ks]), "blocks"


@pytest.mark.parametrize("D", [33, 48])
def test_three_visits_per_workgroup(D):
    """n = 3 * grid + 5 with four sub-steps per visit: every persistent workgroup makes at least three visits -- both parities of
    the double-buffered results, the resets between visits, the first requests of the next trajectory under the last sub-step --
    against the same launch on chunks of at most one grid (one visit per workgroup), bit for bit"""
    from semiclassical_amd._lib import lib
    grid = lib.sc_step_grid(10 ** 6, D)
    n = 3 * grid + 5
    _, y = inp.reference_state(D, n, stream=5, amplitude=AMPLITUDE)
    assert pairs._row_dominance(D, y) < 0.25
    a = _visit(D, y, 4)
    assert a._gstep == grid and int(a._multi["bad"].item()) == 0
    whole = _snapshot(a) + [a._mono.reshape(n, -1)] + [x.reshape(n, -1) for j in range(3) for x in _mid(a, j)]
    for i0 in range(0, n, grid):
        i1 = min(n, i0 + grid)
        c = _visit(D, np.ascontiguousarray(y[:, i0:i1]), 4)
        assert int(c._multi["bad"].item()) == 0
        part = _snapshot(c) + [c._mono.reshape(i1 - i0, -1)] + [x.reshape(i1 - i0, -1) for j in range(3) for x in _mid(c, j)]
        for k, (x, z) in enumerate(zip(whole, part)):
            assert torch.equal(x.reshape(n, -1)[i0:i1], z.reshape(i1 - i0, -1)), (i0, k)


def _as_model(D, n, seed=0):
    import bench
    from semiclassical_amd import potentials as P, propagators as PR
    torch.set_default_dtype(torch.float64)
    omega, chi, nac, q0, _ = bench.as60_model(D)
    G = torch.diag(omega)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, generator=torch.Generator().manual_seed(seed + D))
    return prop, P.MorsePotential(omega, chi.clone(), nac)


def _run(D, n, nt, setup):
    prop, pot = _as_model(D, n)
    setup(prop)
    prop.kernel_timing = True
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
    moments = torch.zeros((nt, 6), dtype=torch.float64, device=prop.device)
    blocks = torch.zeros((nt, 4, 4), dtype=torch.float64, device=prop.device)
    prop.run(pot, 4.0, nt, slots=slots, moments=moments, blocks=blocks)
    prop.synchronize()
    return prop, (slots[:, :4].clone(), moments, blocks, prop.y.clone())


def _visits_of(ks):
    def setup(prop):
        prop.visit_steps, prop.visit_min_bytes = ks, 0     # 300 trajectories are far below the size from which run() takes visits
    return setup


def _no_pairs(prop):
    prop.pair_steps = False


@pytest.mark.parametrize("nt,want", [(5, (1, 0, 1)), (6, (1, 1, 0)), (7, (2, 0, 0)), (9, (2, 0, 1))])
def test_tail_of_run(nt, want):
    """AS model (diagonal blocks, as run() requires), D = 33, n = 300, visit_steps = 4: nt = 5, 6, 7, 9 end in a single step, a
    pair, a visit of three, and a single step after two visits -- never a visit longer than the steps left (`want`: launches of
    visits, pairs and single steps).  Slots, moments, blocks, the final state and the time against one launch per step, bit for bit"""
    a, got = _run(33, 300, nt, _visits_of(4))
    b, ref = _run(33, 300, nt, _no_pairs)
    times = a.kernel_times_ms()
    print(nt, {k: len(v) for k, v in times.items()})
    assert a._multi is not None and b._multi is None
    for k, (x, z) in enumerate(zip(got, ref)):
        assert torch.equal(x, z), (nt, k)
    assert a.t == b.t and a._nsteps == b._nsteps == nt
    assert int(a._multi["bad"].item()) == 0
    assert tuple(len(times.get(label, [])) for label in ("hk_step_visit", "hk_step_pair", "hk_step")) == want
    assert len(b.kernel_times_ms()["hk_step"]) == nt


def test_visit_steps_two_is_the_pair_sequence():
    """visit_steps = 2 launches what run() launched before there were visits: seven steps are three pairs and a single step, each
    row of the slots from one correlate launch"""
    a, got = _run(33, 300, 7, _visits_of(2))
    b, ref = _run(33, 300, 7, _no_pairs)
    counts = {k: len(v) for k, v in a.kernel_times_ms().items()}
    print(counts)
    assert counts == {"hk_correlate": 7, "hk_step_pair": 3, "hk_step": 1}
    for x, z in zip(got, ref):
        assert torch.equal(x, z)


def test_what_run_takes_by_default():
    """three steps per visit for 32 < D <= 64 once the blocks of the ensemble exceed the memory-side cache, pairs below that size"""
    prop, pot = _as_model(33, 300)
    desc = prop._potential_descriptor(pot, 4.0)
    assert prop.visit_steps == 3 and prop._visit_steps_for(desc) == 2
    prop.visit_min_bytes = 32 * 33 * 33 * 300
    assert prop._visit_steps_for(desc) == 3
    prop.visit_steps = 7                       # more than the library has: the longest it supports
    assert prop._visit_steps_for(desc) == 4


def _shifted_blocks(D, n):
    """the fixture of tests/test_pair_no_mid_store_gpu.py: cyclically shifted blocks, every leading pivot of the register elimination
    is zero in every sub-step"""
    _, y = inp.reference_state(D, n)
    gen = torch.Generator().manual_seed(3)
    shift = torch.roll(torch.eye(D), 11, dims=1).unsqueeze(2).expand(-1, -1, n).clone() * (1.0 + 0.1 * torch.rand(D, D, n, generator=gen))
    zero = torch.zeros(D, D, n)
    for k, blk in enumerate([shift, zero, zero, shift.clone()]):
        y[2 * D + k * D * D: 2 * D + (k + 1) * D * D] = blk.reshape(D * D, n).numpy()
    return y


@pytest.mark.parametrize("D,ks", [(60, 4), (48, 3)])
def test_weak_pivot_in_the_last_sub_step_finds_its_blocks(D, ks):
    """the fix-up launch of the last sub-step reads M(k + ks) from memory, where the last sub-step must have put it although nothing
    was stored in between: state, action, blocks and determinants equal the one-step path; every trajectory is counted once per
    intermediate sub-step, and the next check raises (an intermediate determinant cannot be repaired: the contract of pairs).
    The branch SIGN is not compared: it is tracked from determinant to determinant, the intermediate ones are by construction the
    unrepaired zeros of a zero leading pivot, and over ks = 4 steps the repaired determinants of the one-step path cross the
    branch cut once (measured on MI355X: all 50 signs -1 there, +1 here) -- which is why such a run raises instead of returning"""
    from semiclassical_amd import _lib
    n = 50
    y = _shifted_blocks(D, n)
    a = _visit(D, y, ks)
    b, pot = inp.engine(D, y)
    for _ in range(ks):
        b.step(pot, inp.DT)
    torch.cuda.synchronize()
    b._set_mono_layout(_lib.SC_MONO_TILED16)
    torch.cuda.synchronize()
    bad = int(a._multi["bad"].item())
    print(D, ks, "unrepaired", bad, "of", n)
    for name in ("_qp", "_act", "_mono"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(torch.view_as_real(a._c2), torch.view_as_real(b._c2))
    assert bad == (ks - 1) * n
    with pytest.raises(_lib.EngineError):
        a.synchronize()


@pytest.mark.parametrize("D", [17, 20])
def test_two_tiles_keep_pairs(D):
    """NR = 2 (D <= 32) has no kernel for more than two steps per visit: the library says so, run() takes pairs whatever
    visit_steps asks for, and sc_hk_step_visit with two steps is sc_hk_step_multi: equal to two single steps on dense blocks"""
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import check, lib, ptr
    _, y = inp.reference_state(D, inp.NTRAJ, amplitude=AMPLITUDE)
    a, pot = inp.engine(D, y)
    a.visit_min_bytes = 0
    desc = a._potential_descriptor(pot, inp.DT)
    assert a._visit_steps_for(desc) == 2
    a._launch_step_pair(desc, inp.DT)              # scratch and layout
    torch.cuda.synchronize()
    for ks in (3, 4):
        assert not lib.sc_hk_step_visit_supported(desc, a._state, a._hk, ks)
        assert lib.sc_hk_step_visit(desc, a._state, a._hk, a._multi["ms"], inp.DT, ptr(a._multi["epart"]), ks, a._stream()) == -2      # SC_ERR_UNSUPPORTED
    assert lib.sc_hk_step_visit_supported(desc, a._state, a._hk, 2)
    check(lib.sc_hk_step_visit(desc, a._state, a._hk, a._multi["ms"], inp.DT, ptr(a._multi["epart"]), 2, a._stream()))
    torch.cuda.synchronize()
    b, _ = inp.engine(D, y)
    for _ in range(4):
        b.step(pot, inp.DT)
    torch.cuda.synchronize()
    b._set_mono_layout(_lib.SC_MONO_TILED16)
    torch.cuda.synchronize()
    assert int(a._multi["bad"].item()) == 0
    pairs._assert_same_bits(a, b)
