"""The sqrt branch tracker (reference propagators.py:1006-1066) on every prefactor path of the engine and its fix-ups.

Every case starts from a hand-made state (tests/branch_cases.py), takes the determinants z of the next step from the oracle,
and gives the engine and the oracle the same mirrored predecessor: prev = conj(z)(1 + d) where Re z < 0 (must flip), z(1 + d)
(must not), a prev with Re > 0 or a z with Re > 0 (must not), with random incoming signs.  The signs must then agree bit for
bit, the determinants to 1e-10, and the correlation functions to 1e-9.  Each case asserts that it saw flips in both
directions and that the route it is named after was taken."""
import numpy as np
import pytest
import torch

from tests import branch_cases as B
from tests import cases

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

C_TOL, CORR_TOL = 1e-10, 1e-9
WM_CORR_TOL = 1e-8          # the WM correlation terms of random blocks reach 1e52: their sums cancel more (as tests/test_wm_gpu.py)


def cnp(x):
    return x.detach().cpu().numpy()


def _engine(case, ref, exploit_separability=False):
    from semiclassical_amd import propagators as PR
    if case.wm:
        prop = PR.WaltonManolopoulosPropagator(case.Gi, case.Gi, *case.wm, device="cuda")
    else:
        prop = PR.HermanKlukPropagator(case.Gi, case.Gi, device="cuda", exploit_separability=exploit_separability)
    prop.set_initial_conditions(case.q0, case.p0, case.Gi, ref.zi, ref.probi)
    return prop


def _install(prop, setup):
    for key, (_, prev, sgn, _) in setup.items():
        s_attr, z_attr = prop._TRACKED[key]
        getattr(prop, z_attr).copy_(prev.to(prop.device))
        getattr(prop, s_attr).copy_(sgn.to(prop.device))


def _compare_trackers(prop, ref):
    for key, (s_attr, z_attr) in prop._TRACKED.items():
        want_s = ref.tracker.signs(key).real.numpy()
        assert np.array_equal(cnp(getattr(prop, s_attr)), want_s), key
        want_z = ref.tracker.state[key]["previous"].numpy()
        assert cases.rel_err(cnp(getattr(prop, z_attr)), want_z) < C_TOL, key


def _mirrored_step(case, make_blocks, n, seed=1, route=None, without_flags=False, pre_steps=0, exploit_separability=False,
                   premise_keys=None):
    """one engine step from a hand-made state with mirrored predecessors, against the oracle"""
    ref = case.oracle(n, seed)
    prop = _engine(case, ref, exploit_separability)
    if without_flags:
        prop._state.flags = None
    pot = case.engine_potential()
    gen = torch.Generator().manual_seed(seed)
    y = B.with_blocks(ref.y, case.D, make_blocks(case.D, n, gen, torch.diagonal(case.Gi)))
    ref.y = y.clone()
    prop.y = y.cuda()
    for _ in range(pre_steps):          # the engine keeps whatever basis / layout its step left the blocks in
        ref.step(case.oracle_pot, case.dt)
        prop.step(pot, case.dt)
    setup = B.mirrored_setup(ref, ref.y, case.oracle_pot, case.dt, seed, premise_keys=premise_keys)
    want = B.oracle_step_from(ref, ref.y, setup, case.oracle_pot, case.dt)
    _install(prop, setup)
    prop._flags[-2] = -1                # the flag counter of the step (left alone by the paths that do not flag)
    prop.step(pot, case.dt)
    torch.cuda.synchronize()
    if route is not None:
        prop._branch_test_dt = case.dt
        route(prop, pot)
    _compare_trackers(prop, want)
    tol = WM_CORR_TOL if case.wm else CORR_TOL
    assert cases.rel_err(prop.autocorrelation(), want.autocorrelation()) < tol
    assert cases.rel_err(prop.ic_correlation(pot), want.ic_correlation(case.oracle_pot)) < tol
    return prop


# ---------------------------------------------------------------------------------------------------- route checks
def _flagged(prop):
    return int(prop._flags[-2].item())


def tiled(fixup):
    def check(prop, pot):
        from semiclassical_amd import _lib
        assert prop._state.mono_layout == _lib.SC_MONO_TILED16
        flagged = _flagged(prop)
        assert flagged == prop.ntraj if fixup else 0 <= flagged < prop.ntraj, flagged
    return check


def fixed_order(fixup):
    """sep16 / lin / dense-mono: the flag counter of the step; the shifted blocks send every trajectory to the fix-up"""
    def check(prop, pot):
        flagged = _flagged(prop)
        assert flagged == prop.ntraj if fixup else 0 <= flagged < prop.ntraj, flagged
        assert int(prop._flags[:-2].abs().sum().item()) == 0          # the fix-up cleared the flags it served
    return check


def w16(prop, pot):
    assert 13 <= prop.dim <= 16 and bool(prop._pre.diag) and _flagged(prop) == -1     # no counter: the kernel pivots by itself


def lin(fixup):
    def check(prop, pot):
        from semiclassical_amd import _lib
        desc = prop._potential_descriptor(pot, prop._branch_test_dt)
        assert desc.kind == _lib.SC_POT_HARMONIC_DENSE and bool(desc.lin_prop) and prop.dim <= 16
        fixed_order(fixup)(prop, pot)
    return check


def general(prop, pot):
    """hk_step_kernel: no flag array, or widths that are not diagonal -- no fast kernel, no counter"""
    assert prop._state.flags is None or not bool(prop._pre.diag)
    assert int(prop._flags[-2].item()) == -1


def shortcut(prop, pot):
    assert prop._mono_stale and prop._mono_is_diag


def modal(prop, pot):
    assert prop._modal_basis is not None


def wm_route(rerun):
    def check(prop, pot):
        flagged = int(prop._wm_flags[-1].item())
        assert (0 < flagged < prop.ntraj) if rerun else flagged >= 0, flagged
    return check


ROUTES = {
    "fast": tiled(False), "fast-fixup": tiled(True), "w16": w16, "sep16": fixed_order(False), "sep16-fixup": fixed_order(True),
    "lin": lin(False), "lin-fixup": lin(True), "general": general, "diag": shortcut, "modal": modal,
    "dense-mono": fixed_order(False), "dense-mono-fallback": fixed_order(True), "dense-any": None,
    "wm": wm_route(False), "wm-rerun": wm_route(True),
}


@pytest.mark.parametrize("name,route,make_case,make_blocks,n,kw", B.ONE_STEP, ids=[r[0] for r in B.ONE_STEP])
def test_one_step(name, route, make_case, make_blocks, n, kw):
    _mirrored_step(make_case(), make_blocks, n, route=ROUTES[route], **kw)


# ---------------------------------------------------------------------------------------------------- whole loop


@pytest.mark.parametrize("name,make_case,nt,normal_modes", B.WHOLE_LOOP, ids=[r[0] for r in B.WHOLE_LOOP])
def test_whole_loop(name, make_case, nt, normal_modes):
    """sc_hk_run (separable, constant Hessian, normal modes): the predecessor of the FIRST step of the run is mirrored; the final
    signs, C(t) and k_ic(t) of all nt steps against the oracle's loop"""
    from oracle import sc_oracle as orc
    case, n, seed = make_case(), 256, 2
    ref = case.oracle(n, seed)
    prop = _engine(case, ref)
    pot = case.engine_potential()
    gen = torch.Generator().manual_seed(seed)
    y = B.with_blocks(ref.y, case.D, B.dense_blocks(case.D, n, gen, torch.diagonal(case.Gi)))
    setup = B.mirrored_setup(ref, y, case.oracle_pot, case.dt, seed)
    want = B.oracle_step_from(ref, y, setup, case.oracle_pot, case.dt, steps=0)
    rc, rk = orc.run_loop(want, case.oracle_pot, case.dt, nt)
    prop.y = y.cuda()
    _install(prop, setup)
    desc = prop._potential_descriptor(pot, case.dt)
    assert prop._whole_loop_applies(desc)
    assert (prop._modal_constants(pot, desc, case.dt) is not None and nt >= prop.normal_modes_from) == normal_modes
    c, k = prop.run(pot, case.dt, nt)
    _compare_trackers(prop, want)
    assert cases.rel_err(c, rc) < CORR_TOL and cases.rel_err(k, rk) < CORR_TOL


# ---------------------------------------------------------------------------------------------------- two-step pair
def _pair_run(case, y, ref, setup_prev, setup_sgn):
    from semiclassical_amd import _lib
    prop = _engine(case, ref)
    pot = case.engine_potential()
    prop.y = y.cuda()
    prop._c2.copy_(setup_prev.cuda())
    prop._sgn.copy_(setup_sgn.cuda())
    desc = prop._potential_descriptor(pot, case.dt)
    prop._launch_step_pair(desc, case.dt)
    torch.cuda.synchronize()
    assert prop._state.mono_layout == _lib.SC_MONO_TILED16
    return prop


@pytest.mark.parametrize("D", [33, 60])
def test_two_step_pair(D):
    """sc_hk_step_multi: the first step's predecessor mirrored, the second step flips by itself (the phase turns by about a
    radian per step); flips at the intermediate step only, at the final step only and at both"""
    case, n, seed = B.morse_case(D), 256, 1
    ref = case.oracle(n, seed)
    gen = torch.Generator().manual_seed(seed)
    y = B.with_blocks(ref.y, D, B.dense_blocks(D, n, gen, torch.diagonal(case.Gi), noise=B.PAIR_NOISE))
    z1, z2, prev, sgn, f1, f2 = B.pair_setup(ref, y, case.oracle_pot, case.dt, seed)
    counts = B.pair_counts(f1, f2)
    assert min(counts.values()) >= B.MIN_PER_CATEGORY, counts
    want = B.oracle_step_from(ref, y, {"prefactorC": (None, prev, sgn, None)}, case.oracle_pot, case.dt, steps=2)
    prop = _pair_run(case, y, ref, prev, sgn)
    assert int(prop._multi["bad"].item()) == 0
    mid_sgn, mid_c2 = cnp(prop._multi["sgn"][:n]), cnp(prop._multi["c2"][:n])
    assert np.array_equal(mid_sgn, (sgn * torch.where(f1, -1.0, 1.0)).numpy())
    assert cases.rel_err(mid_c2, z1.numpy()) < C_TOL
    _compare_trackers(prop, want)
    prop.synchronize()


def test_weak_pivot_in_the_last_sub_step_tracks_against_the_intermediate_step():
    """sc_hk_step_multi, the last sub-step weak in-block and the intermediate one not (tests/branch_cases.py
    weak_last_blocks): the fix-up pass must track the final determinant against the INTERMEDIATE one.  Tracking against the
    value from before the pair drops the flips made at the intermediate step, and nothing would be raised."""
    D, row, col, n, seed, make_case = B.WEAK_LAST
    case = make_case()
    ref = case.oracle(n, seed)
    y = B.with_blocks(ref.y, D, B.weak_last_blocks(ref, case.oracle_pot, case.dt, row, col, seed + 3))
    first, second = B.weak_last_premise(ref, y, case.oracle_pot, case.dt, row, col)
    assert float(first.min()) > 0.25 and float(second.max()) < 1e-9         # weak means below 1/16
    z1, z2, prev, sgn, f1, f2 = B.pair_setup(ref, y, case.oracle_pot, case.dt, seed + 3)
    assert int(f1.sum()) >= B.MIN_PER_CATEGORY
    assert int((B.would_flip(prev, z2) != (f1 ^ f2)).sum()) >= B.MIN_PER_CATEGORY   # the wrong predecessor changes signs
    want = B.oracle_step_from(ref, y, {"prefactorC": (None, prev, sgn, None)}, case.oracle_pot, case.dt, steps=2)
    prop = _pair_run(case, y, ref, prev, sgn)
    assert int(prop._multi["bad"].item()) == 0                              # the intermediate step needed no repair
    assert _flagged(prop) == n                                              # the last one went to the fix-up for all
    _compare_trackers(prop, want)
    prop.synchronize()
