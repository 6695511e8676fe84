"""Discarding trajectories that fail the symplecticity check (sc_discard_mark, sc_term_masked_sums,
HermanKlukPropagator.discard_nonsymplectic, the driver key "discard_nonsymplectic").

Comparison rule for every sum: the reference is the float64 NumPy sum of the exported per-trajectory terms over the HOST's own
mask, and the tolerance is the bound that holds for any two summation orders of the same n terms,
    |gpu - host| <= 2 n 2^-53 sum_i |x_i|   per real component,
x_i the terms for slots and blocks, their squares / products for the moments (the kernel fuses the product into the add, the host
rounds it first: one more rounding per term, inside the bound).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases, engine_cases, symplectic_ref as R
from tests.lib_spy import LibSpy as _Spy

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

U = 2.0 ** -53
# one pass of term_masked_partial_kernel takes 64 workgroups x 256 threads x 4 trajectories: the last size walks the stride loop
# three times and ends in a partial group
SIZES = [1, 3, 4, 5, 255, 257, 1030, 4 * 64 * 256 * 2 + 7]
# one pass of discard_mark_kernel takes 32 workgroups x 256 threads: 8199 trajectories take the stride loop twice
BEYOND_MARK_GRID = 4 * 2048 + 7


# ---------------------------------------------------------------------------------------------------------------- host reference
def host_sums(cq, kq, keep, B=0):
    """the masked sums and the sums of |x| their tolerance is made of: (slot (4,), moments (6,), blocks (B, 4)) twice"""
    from semiclassical_amd import hostmath
    keep = np.asarray(keep, dtype=bool)
    zero = np.zeros(int(keep.sum()))
    cr, ci = cq.real[keep], cq.imag[keep]
    kr, ki = (kq.real[keep], kq.imag[keep]) if kq is not None else (zero, zero)
    cols = [cr, ci, kr, ki]
    prods = [cr * cr, ci * ci, cr * ci, kr * kr, ki * ki, kr * ki]
    total = lambda xs: np.array([x.sum() for x in xs])
    scale = lambda xs: np.array([np.abs(x).sum() for x in xs])
    blocks, bscale = np.zeros((B, 4)), np.zeros((B, 4))
    if B:
        blk = hostmath.error_block(np.arange(len(keep)), B)[keep]
        for b in range(B):
            blocks[b], bscale[b] = total([x[blk == b] for x in cols]), scale([x[blk == b] for x in cols])
    return (total(cols), total(prods), blocks), (scale(cols), scale(prods), bscale)


def assert_within_bound(got, want, scale, n, label):
    bound = 2.0 * n * U * scale
    err = np.abs(np.asarray(got) - want)
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    print(f"{label}: largest |gpu - host| / bound = {worst:.3f}")
    assert np.all(err <= bound), (label, err, bound)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def masked_sums(cq, kq, kept, B, moments):
    """sc_term_masked_sums through the C-ABI -> (slot row (5,), moments (6,) or None, blocks (B, 4) or None) on the host"""
    from semiclassical_amd import _lib
    dev = cq.device
    scratch = torch.full((_lib.lib.sc_term_masked_scratch_doubles(),), np.nan, device=dev)
    slot = torch.full((5,), 7.5, device=dev)
    mom = torch.full((6,), 7.5, device=dev) if moments else None
    blocks = torch.full((B, 4), 7.5, device=dev) if B else None
    _lib.check(_lib.lib.sc_term_masked_sums(_p(cq), _p(kq), _p(kept), cq.shape[0], B, _p(scratch), _p(slot), _p(mom), _p(blocks),
                                            _stream()))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(slot), host(mom), host(blocks)


def synthetic(n, seed):
    rng = np.random.default_rng(seed)
    cq = rng.normal(size=n) + 1j * rng.normal(size=n)
    kq = rng.normal(size=n) + 1j * rng.normal(size=n)
    keep = rng.random(n) < 0.6
    keep[0] = True                       # never an empty sum by accident ...
    if n > 1:
        keep[1] = False                  # ... nor a full mask
    return cq, kq, keep


# ------------------------------------------------------------------------------------------------ 1. the kernel, through the C-ABI
@pytest.mark.parametrize("n", SIZES)
def test_masked_sums_kernel(n):
    """slots, moments and blocks of synthetic terms under a random mask against the host, for every B, with and without moments
    and k terms; the blocks add up to the slot row; column 4 of the slot row is not touched"""
    cq, kq, keep = synthetic(n, 1000 + n)
    d_cq, d_kq = torch.from_numpy(cq).cuda(), torch.from_numpy(kq).cuda()
    d_keep = torch.from_numpy(keep.astype(np.uint8)).cuda()
    for B in (0, 2, 8, 64):
        for moments in (False, True):
            for has_k in (True, False):
                slot, mom, blocks = masked_sums(d_cq, d_kq if has_k else None, d_keep, B, moments)
                want, scale = host_sums(cq, kq if has_k else None, keep, B)
                label = f"n={n} B={B} moments={moments} k={has_k}"
                assert slot[4] == 7.5, "column 4 of the slot row was written"
                assert_within_bound(slot[:4], want[0], scale[0], n, label + " slots")
                if moments:
                    assert_within_bound(mom, want[1], scale[1], n, label + " moments")
                if B:
                    assert_within_bound(blocks, want[2], scale[2], n, label + " blocks")
                    assert_within_bound(blocks.sum(axis=0), slot[:4], scale[0], n, label + " sum of blocks vs slots")
                if not has_k:
                    assert np.all(slot[2:4] == 0.0) and (mom is None or np.all(mom[3:] == 0.0))
                    assert blocks is None or np.all(blocks[:, 2:] == 0.0)


@pytest.mark.parametrize("n", SIZES)
def test_masked_sums_bits(n):
    """two launches give the same bits; an all-zero mask gives exact zeros; inf and NaN at every cleared position never reach an
    accumulator: all outputs finite and bit for bit those of the same launch with zeros planted there"""
    cq, kq, keep = synthetic(n, 2000 + n)
    d_keep = torch.from_numpy(keep.astype(np.uint8)).cuda()
    up = lambda x: torch.from_numpy(x).cuda()
    first = masked_sums(up(cq), up(kq), d_keep, 8, True)
    again = masked_sums(up(cq), up(kq), d_keep, 8, True)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    nobody = masked_sums(up(cq), up(kq), torch.zeros(n, dtype=torch.uint8, device="cuda"), 8, True)
    assert np.all(nobody[0][:4] == 0.0) and np.all(nobody[1] == 0.0) and np.all(nobody[2] == 0.0)
    bad_c, bad_k, zero_c, zero_k = cq.copy(), kq.copy(), cq.copy(), kq.copy()
    gone = np.flatnonzero(~keep)
    poison = np.array([np.inf, np.nan + 0j, -np.inf * 1j, complex(np.nan, np.inf)])
    bad_c[gone] = poison[np.arange(len(gone)) % 4]
    bad_k[gone] = poison[(np.arange(len(gone)) + 1) % 4]
    zero_c[gone], zero_k[gone] = 0.0, 0.0
    for B, moments in ((8, True), (64, False), (0, True)):
        poisoned = masked_sums(up(bad_c), up(bad_k), d_keep, B, moments)
        zeroed = masked_sums(up(zero_c), up(zero_k), d_keep, B, moments)
        for a, b in zip(poisoned, zeroed):
            assert (a is None and b is None) or (np.all(np.isfinite(a)) and np.array_equal(a, b))


def test_bad_arguments_are_refused():
    from semiclassical_amd import _lib
    lib, n = _lib.lib, 16
    cq = torch.zeros(n, dtype=torch.complex128, device="cuda")
    kept = torch.ones(n, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(lib.sc_term_masked_scratch_doubles(), device="cuda")
    slot, blocks = torch.zeros(5, device="cuda"), torch.zeros((64, 4), device="cuda")
    sums = lambda *a: lib.sc_term_masked_sums(*a, _stream())
    assert sums(_p(cq), None, _p(kept), n, 8, _p(scratch), _p(slot), None, _p(blocks)) == 0
    for B in (1, 3, 6, 128, -2):
        assert sums(_p(cq), None, _p(kept), n, B, _p(scratch), _p(slot), None, _p(blocks)) != 0, B
    assert sums(None, None, _p(kept), n, 0, _p(scratch), _p(slot), None, None) != 0
    assert sums(_p(cq), None, None, n, 0, _p(scratch), _p(slot), None, None) != 0
    assert sums(_p(cq), None, _p(kept), n, 0, None, _p(slot), None, None) != 0
    assert sums(_p(cq), None, _p(kept), n, 0, _p(scratch), None, None, None) != 0
    assert sums(_p(cq), None, _p(kept), n, 8, _p(scratch), _p(slot), None, None) != 0          # blocks wanted, no buffer
    dev = torch.zeros((n, 3), device="cuda")
    at = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    mark = lambda *a: lib.sc_discard_mark(*a, _stream())
    assert mark(_p(dev), n, 1e-3, 0, _p(kept), _p(at), _p(count)) == 0
    for tol in (0.0, -1.0, float("nan")):
        assert mark(_p(dev), n, tol, 0, _p(kept), _p(at), _p(count)) != 0, tol
    assert mark(None, n, 1e-3, 0, _p(kept), _p(at), _p(count)) != 0
    assert mark(_p(dev), n, 1e-3, 0, None, _p(at), _p(count)) != 0
    assert mark(_p(dev), n, 1e-3, 0, _p(kept), None, _p(count)) != 0
    assert mark(_p(dev), n, 1e-3, 0, _p(kept), _p(at), None) != 0
    torch.cuda.synchronize()
    assert int(count.item()) == n and bool(kept.all())


# ------------------------------------------------------------------------------------------------------------------- 2. the mark
def _separable(D):
    """widths and a Morse potential of D modes whose frequencies are those widths"""
    from semiclassical_amd import potentials as P
    omega = torch.linspace(0.002, 0.015, D) if D > 1 else torch.tensor([0.01])
    nac = torch.from_numpy(np.random.default_rng(D).normal(0, 1e-3, D))
    return torch.diag(omega), P.MorsePotential(omega, torch.full((D,), 0.02), nac)


def bare_propagator(D, n):
    """an HK propagator of n trajectories in D dimensions whose state the tests overwrite through the `y` setter"""
    from semiclassical_amd import propagators as PR
    G, pot = _separable(D)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    zero = torch.zeros(D)
    prop.set_initial_conditions(zero, zero, G, torch.zeros((2 * D, n)), torch.ones(n))
    return prop, pot


def planted_blocks(n, D, subset, factor=1.3):
    """identity blocks, Mqq scaled by `factor` for the subset: E2 = (factor - 1) 1, deviation 0.3 in any scale"""
    blocks = np.zeros((n, 4, D, D))
    blocks[:, 0] = blocks[:, 3] = np.eye(D)
    blocks[subset, 0] *= factor
    return blocks


@pytest.mark.parametrize("D,n", [(5, 3), (5, 24), (5, BEYOND_MARK_GRID), (16, 3), (16, 24), (17, 3), (17, 24), (33, 3), (33, 24)])
def test_mark(D, n):
    """finite defects planted through the y setter, and one trajectory with a NaN block element: the mask is exactly the
    complement, discarded_at the step count, the count matches, a second mark at a huge tolerance revives nobody, and the
    correlation functions of this state are the host's masked sums of the exported terms (the state is marked and correlated,
    never stepped)"""
    prop, pot = bare_propagator(D, n)
    for _ in range(2):
        prop.step(pot, 2.0)                                  # a step count other than 0
    assert prop._kept is None and bool(prop.kept.all()) and prop.kept_count() == n
    assert prop.kept.dtype == torch.bool and prop.discarded_at.dtype == torch.int32 and bool((prop.discarded_at == -1).all())
    subset = np.arange(n) % 3 == 1
    blocks = planted_blocks(n, D, subset)
    blocks[0, 2, D - 1, 0] = np.nan                          # trajectory 0: not in the subset, not finite
    prop.y = torch.from_numpy(R.y_from_blocks(blocks))
    gone = subset.copy()
    gone[0] = True
    eps = prop.discard_nonsymplectic(1e-3)
    assert eps.shape == (n,) and torch.equal(eps, prop.symplectic_deviation())
    eps = eps.cpu().numpy()
    assert np.isposinf(eps[0]) and np.all(eps[~gone] == 0.0) and np.all(np.abs(eps[subset] - 0.3) < 1e-12)
    for tol in (None, 1e3):                                  # the second mark: sticky
        if tol is not None:
            prop.discard_nonsymplectic(tol)
        assert np.array_equal(prop.kept.cpu().numpy(), ~gone)
        assert np.array_equal(prop.discarded_at.cpu().numpy(), np.where(gone, 2, -1))
        assert prop.kept_count() == int((~gone).sum())
    c = prop.autocorrelation()
    k = prop.ic_correlation(pot)
    cq, kq = prop._cq.cpu().numpy(), prop._kq.cpu().numpy()
    want, scale = host_sums(cq, kq, ~gone)
    assert_within_bound([c.real, c.imag, k.real, k.imag], want[0], scale[0], n, f"D={D} n={n}")
    assert np.all(scale[0][:2] > 0), "the kept terms are all zero: the comparison says nothing"
    assert prop._slot_host[4] == 0.0


# -------------------------------------------------------------------------------------------------------------- 3. state untouched
def test_mark_leaves_the_state_alone():
    """hk_as33: ten steps with a mark after step 5 leave y, c2 and the sign tracker bit for bit as ten steps without it"""
    g = cases.load("hk_as33")
    pot, dt = engine_cases.engine_potential(g), float(g["dt"])
    marked, plain = engine_cases.engine_propagator(g), engine_cases.engine_propagator(g)
    for step in range(10):
        if step == 5:
            tol = float(torch.median(marked.symplectic_deviation()))
            marked.discard_nonsymplectic(tol)
        marked.step(pot, dt)
        plain.step(pot, dt)
    assert 0 < marked.kept_count() < marked.ntraj and plain._kept is None
    assert torch.equal(marked.y, plain.y) and torch.equal(marked._c2, plain._c2) and torch.equal(marked._sgn, plain._sgn)
    assert marked._nsteps == plain._nsteps == 10


# ------------------------------------------------------------------------------------------ 4. the routes of run() under a mask
NT, NB = 7, 8


def prepared(name, tol=None, steps=3, **attrs):
    """the fixture's propagator after `steps` steps at its own time step, marked at `tol` (default: the median of the deviations
    the check returns) -> (propagator, potential, dt, tol, the host's own mask)"""
    g = cases.load(name)
    pot, dt = engine_cases.engine_potential(g), float(g["dt"])
    prop = engine_cases.engine_propagator(g)
    for key, value in attrs.items():
        setattr(prop, key, value)
    for _ in range(steps):
        prop.step(pot, dt)
    if tol is None:
        tol = float(torch.median(prop.symplectic_deviation()))
    eps = prop.discard_nonsymplectic(tol).cpu().numpy()
    keep = eps <= tol
    # neither an empty nor a full mask
    assert prop.ntraj / 4 <= keep.sum() <= 3 * prop.ntraj / 4, (name, int(keep.sum()), prop.ntraj)
    assert np.array_equal(prop.kept.cpu().numpy(), keep) and prop.kept_count() == int(keep.sum())
    return prop, pot, dt, tol, keep


def run_masked(prop, pot, dt, **kw):
    slots = torch.full((NT, 5), 7.5, device=prop.device)
    mom = torch.zeros((NT, 6), device=prop.device)
    blocks = torch.zeros((NT, NB, 4), device=prop.device)
    prop.run(pot, dt, NT, slots=slots, moments=mom, blocks=blocks, **kw)
    prop.synchronize()
    assert bool((slots[:, 4] == 7.5).all()), "column 4 of the slot rows was written"
    return slots.cpu().numpy()[:, :4], mom.cpu().numpy(), blocks.cpu().numpy()


def step_by_step(prop, pot, dt, keep):
    """NT times (ic_correlation, host sums of the exported terms over the host's mask, step) -> per step (got (4,), want, scale)"""
    rows = []
    for _ in range(NT):
        c = prop.autocorrelation()
        k = prop.ic_correlation(pot)
        got = np.array([c.real, c.imag, k.real, k.imag])
        rows.append((got,) + host_sums(prop._cq.cpu().numpy(), prop._kq.cpu().numpy(), keep, NB))
        prop.step(pot, dt)
    prop.synchronize()
    return rows


def assert_run_against_host(run, rows, n, label):
    slots, mom, blocks = run
    for k, (_, want, scale) in enumerate(rows):
        assert_within_bound(slots[k], want[0], scale[0], n, f"{label} step {k} slots")
        assert_within_bound(mom[k], want[1], scale[1], n, f"{label} step {k} moments")
        assert_within_bound(blocks[k], want[2], scale[2], n, f"{label} step {k} blocks")
        assert np.all(scale[0] > 0), "a column of kept terms is all zero: the comparison says nothing"


def test_routes_agree_d33(monkeypatch):
    """hk_as33 under the natural mask of the median: one launch per step, pairs and three-step visits give the same bits, and
    each agrees with the step-by-step host sums"""
    routes = [("single", {"pair_steps": False}, "sc_hk_step"), ("pairs", {}, "sc_hk_step_multi"),
              ("visits", {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit")]
    tol, runs = None, []
    for label, attrs, entry in routes:
        prop, pot, dt, tol, keep = prepared("hk_as33", tol, **attrs)
        spy = _Spy(monkeypatch)
        runs.append(run_masked(prop, pot, dt))
        monkeypatch.undo()
        assert spy.seen.get(entry, 0) > 0, f"{label}: {entry} did not run"
        assert spy.seen.get("sc_term_masked_sums", 0) == NT and "sc_reduce_slot" not in spy.seen and "sc_term_blocks" not in spy.seen
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)
    prop, pot, dt, _, keep2 = prepared("hk_as33", tol)
    assert np.array_equal(keep, keep2)
    rows = step_by_step(prop, pot, dt, keep)
    for (label, _, _), run in zip(routes, runs):
        assert_run_against_host(run, rows, prop.ntraj, label)


def test_whole_loop_case_d5(monkeypatch):
    """hk_as5_chi002, normally ONE launch: under a mask run() goes step by step and agrees with autocorrelation() /
    ic_correlation() / step() called one at a time under the same mask; without a mask it still is the one launch and the golden"""
    prop, pot, dt, tol, keep = prepared("hk_as5_chi002")
    spy = _Spy(monkeypatch)
    run = run_masked(prop, pot, dt)
    monkeypatch.undo()
    assert "sc_hk_run" not in spy.seen and "sc_hk_run_m" not in spy.seen and spy.seen.get("sc_term_masked_sums", 0) == NT
    twin, _, _, _, keep2 = prepared("hk_as5_chi002", tol)
    assert np.array_equal(keep, keep2)
    rows = step_by_step(twin, pot, dt, keep)
    assert_run_against_host(run, rows, prop.ntraj, "as5")
    for k, (got, want, scale) in enumerate(rows):             # the one-at-a-time calls themselves, and run() against them
        assert_within_bound(got, want[0], scale[0], prop.ntraj, f"as5 one at a time, step {k}")
        assert_within_bound(run[0][k], got, scale[0], prop.ntraj, f"as5 run() against one at a time, step {k}")
    assert torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2)
    # no mask: the route and the result of always
    g = cases.load("hk_as5_chi002")
    plain = engine_cases.engine_propagator(g)
    spy = _Spy(monkeypatch)
    c, k = plain.run(pot, dt, int(g["nt"]), float(g["E0"]))
    monkeypatch.undo()
    assert plain._kept is None and spy.seen.get("sc_hk_run", 0) == 1 and "sc_term_masked_sums" not in spy.seen
    assert cases.rel_err(c, g["cauto"]) < 1e-9 and cases.rel_err(k, g["kic"]) < 1e-9


def test_wm_masked_sums():
    """wm_as5_chi002: masked slots, moments and blocks against the host sums of the exported WM terms"""
    prop, pot, dt, tol, keep = prepared("wm_as5_chi002")
    run = run_masked(prop, pot, dt)
    twin, _, _, _, keep2 = prepared("wm_as5_chi002", tol)
    assert np.array_equal(keep, keep2)
    rows = step_by_step(twin, pot, dt, keep)
    assert_run_against_host(run, rows, prop.ntraj, "wm")
    for k, (got, want, scale) in enumerate(rows):
        assert_within_bound(got, want[0], scale[0], prop.ntraj, f"wm one at a time, step {k}")


def test_normal_mode_basis():
    """hk_coumarin_harmonic (constant dense Hessian, D = 51: the blocks live in normal-mode coordinates), 32 trajectories.  The
    monodromy matrix of a constant Hessian is the same for every trajectory, so the deviations are all equal and a median cannot
    split them: the defect of test_mark (Mqq scaled by 1.3, which commutes with the change of basis) is planted for a subset
    instead, in the blocks as they lie.  The mark works through the Cartesian copy, the masked sums are the host's, and the later
    steps keep the bits of a twin that was never marked."""
    g = cases.load("hk_coumarin_harmonic")
    pot, dt = engine_cases.engine_potential(g), float(g["dt"])
    n = 32
    subset = np.arange(n) % 3 == 1
    props = [engine_cases.engine_propagator(g, select=slice(0, n)) for _ in range(2)]
    for prop in props:
        for _ in range(3):
            prop.step(pot, dt)
        assert prop._modal_basis is not None, "the normal-mode step was not taken"
        prop._mono[torch.from_numpy(subset).to(prop.device), 0] *= 1.3
    marked, plain = props
    eps = marked.discard_nonsymplectic(1e-3).cpu().numpy()
    assert marked._modal_basis is not None
    assert np.all(eps[subset] > 0.1) and np.all(eps[~subset] < 1e-5)
    assert np.array_equal(marked.kept.cpu().numpy(), ~subset) and marked.kept_count() == int((~subset).sum())
    assert np.array_equal(marked.discarded_at.cpu().numpy(), np.where(subset, 3, -1))
    c = marked.autocorrelation()
    k = marked.ic_correlation(pot)
    want, scale = host_sums(marked._cq.cpu().numpy(), marked._kq.cpu().numpy(), ~subset)
    assert_within_bound([c.real, c.imag, k.real, k.imag], want[0], scale[0], n, "coumarin")
    assert np.all(scale[0] > 0)
    for prop in props:
        for _ in range(2):
            prop.step(pot, dt)
    assert torch.equal(marked.y, plain.y) and torch.equal(marked._c2, plain._c2) and torch.equal(marked._sgn, plain._sgn)


def test_graph_replay_is_refused_under_a_mask():
    prop, pot, dt, _, _ = prepared("hk_as33")
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, dt, 4, use_graph=True)
    assert prop._nsteps == 3


def test_standard_errors_under_a_mask():
    """run(standard_errors=True) under a mask: sigma = finalize_moments of the host's masked sums and moments with the UNCHANGED
    N.  sigma^2 = (N S - m^2) / (N - 1), so with the bounds bS, bm of the comparison rule on S and m
        |sigma^2_gpu - sigma^2_host| <= (N bS + (2 |m| + bm) bm) / (N - 1) =: b2,   |sigma_gpu - sigma_host| <= b2 / sigma_host
    (|sqrt a - sqrt b| <= |a - b| / sqrt b), plus 8 roundings of the evaluation itself."""
    from semiclassical_amd import propagators as PR
    prop, pot, dt, tol, keep = prepared("hk_as33")
    N = prop._ntraj_norm
    assert N == prop.ntraj
    C, k, sC, sk = prop.run(pot, dt, NT, standard_errors=True)
    twin, _, _, _, _ = prepared("hk_as33", tol)
    rows = step_by_step(twin, pot, dt, keep)
    slots = np.zeros((NT, 5))
    slots[:, :4] = [want[0] for _, want, _ in rows]
    mom = np.array([want[1] for _, want, _ in rows])
    wC, wk = PR.HermanKlukPropagator.finalize_moments(torch.from_numpy(slots), mom, 3 * dt, dt, 0.0, N)
    for j, (_, want, scale) in enumerate(rows):
        bm, bS = 2.0 * N * U * scale[0], 2.0 * N * U * scale[1]
        for got, ref, (im, iS) in ((sC[j].real, wC[j].real, (0, 0)), (sC[j].imag, wC[j].imag, (1, 1)),
                                   (sk[j].real, wk[j].real, (2, 3)), (sk[j].imag, wk[j].imag, (3, 4))):
            b2 = (N * bS[iS] + (2.0 * abs(want[0][im]) + bm[im]) * bm[im]) / (N - 1.0)
            assert ref > 0 and abs(got - ref) <= b2 / ref + 8 * U * ref, (j, got, ref)
    # and the one-step counterpart
    sc1, sk1 = twin.standard_errors()
    assert np.isfinite(sc1.real) and np.isfinite(sk1.real) and sc1.real > 0


# ------------------------------------------------------------------------------------------------------------------- 5. the driver
def _as5_task(tmp_path, tag, **extra):
    g = cases.load("hk_as5_chi002")
    model = tmp_path / "AS_model.dat"
    rows = np.vstack((g["omega"] * 219474.63, 0.5 * g["omega"] * g["q0"] ** 2 * np.sign(g["q0"]), g["nac"], np.full(5, 0.02))).T
    np.savetxt(model, rows)
    task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(model)}, "propagator": "HK",
            "batch_size": 512, "num_trajectories": 512, "num_steps": 12, "time_step_fs": 0.1,
            "results": {"correlations": str(tmp_path / f"{tag}.npz")}, "manual_seed": 11}
    task.update(extra)
    return task


def test_driver_discards(tmp_path, caplog):
    """the driver key: the npz carries the kept counts and the flag, C(t) and k(t) are those of a hand-driven loop over the
    propagator API with the same seed, and a second repetition pools with the kept counts added"""
    import logging
    from semiclassical_amd import driver, units
    from semiclassical_amd import propagators as PR
    task = _as5_task(tmp_path, "probe")
    setup = driver.build_problem(task)
    dt = task["time_step_fs"] / units.autime_to_fs

    def fresh():
        prop = driver.make_propagator(task, setup.Gamma_0, "cuda")
        prop.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=512, ntraj_total=512, seed=11, subsequence=0, first_index=0)
        return prop
    probe = fresh()
    for _ in range(8):
        probe.step(setup.potential, dt)
    tol = float(torch.median(probe.symplectic_deviation()))
    assert tol > 0
    # by hand: marks at steps 0, 4, 8, the raw sums of every step
    prop = fresh()
    raw, kept, eps = np.zeros((12, 5)), [], []
    for step in range(12):
        if step % 4 == 0:
            before = prop.kept.cpu().numpy()
            eps.append((prop.discard_nonsymplectic(tol).cpu().numpy(), before))
            kept.append(prop.kept_count())
        prop.autocorrelation()
        prop.ic_correlation(setup.potential)
        raw[step, :4] = prop._slot_host[:4]
        prop.step(setup.potential, dt)
    C, k = PR.HermanKlukPropagator.finalize_slots(torch.from_numpy(raw), 0.0, dt, setup.zero_point_energy)
    assert kept[0] == 512 and 128 <= kept[2] <= 384 and kept[0] >= kept[1] >= kept[2]

    keys = dict(check_symplecticity_every=4, symplecticity_tolerance=tol, discard_nonsymplectic=True)
    with caplog.at_level(logging.INFO, logger="semiclassical_amd.driver"):
        driver.run_semiclassical_dynamics(_as5_task(tmp_path, "one", **keys), device="cuda")
    assert sum("kept " in r.getMessage() and " of 512" in r.getMessage() for r in caplog.records) == 3
    one = dict(np.load(tmp_path / "one.npz"))
    assert bool(one["symplecticity_discard"]) and np.array_equal(one["symplecticity_kept"], kept)
    assert np.array_equal(one["symplecticity_steps"], [0, 4, 8]) and float(one["symplecticity_tolerance"]) == tol
    assert np.array_equal(one["symplecticity_exceeding"], [int((e > tol).sum()) for e, _ in eps])
    # max and mean over the trajectories that were still kept before each mark
    assert np.array_equal(one["symplecticity_max"], [e[b].max() for e, b in eps])
    assert np.allclose(one["symplecticity_mean"], [e[b].mean() for e, b in eps], rtol=1e-12, atol=0)
    assert np.all(np.isfinite(one["symplecticity_max"]))
    assert np.array_equal(one["autocorrelation"], C) and np.array_equal(one["ic_correlation"], k)
    # and it is another estimator than the one without discarding
    driver.run_semiclassical_dynamics(_as5_task(tmp_path, "plain"), device="cuda")
    plain = dict(np.load(tmp_path / "plain.npz"))
    assert not np.array_equal(plain["autocorrelation"], one["autocorrelation"]) and "symplecticity_kept" not in plain
    # two repetitions: the first is the batch above, the counts add
    driver.run_semiclassical_dynamics(_as5_task(tmp_path, "two", num_trajectories=1024, **keys), device="cuda")
    two = dict(np.load(tmp_path / "two.npz"))
    assert int(two["trajectories"]) == 1024 and bool(two["symplecticity_discard"])
    assert two["symplecticity_kept"][0] == 1024 and np.all(two["symplecticity_kept"] >= one["symplecticity_kept"])
    assert np.all(np.diff(two["symplecticity_kept"]) <= 0) and two["symplecticity_kept"][2] < 1024
    # a later run without the key must not be pooled into that file
    late = _as5_task(tmp_path, "two", results={"correlations": str(tmp_path / "two.npz"), "overwrite": False})
    late.pop("manual_seed")
    with pytest.raises(driver.ConfigurationError, match="discard_nonsymplectic"):
        driver.run_semiclassical_dynamics(late, device="cuda")
