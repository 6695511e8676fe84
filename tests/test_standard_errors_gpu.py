"""Monte-Carlo standard errors of C_auto(t) and k_ic(t): the per-step second-moment sums of run(..., moments=...) on every route
against the six sums formed in torch from the engine's own per-trajectory terms, C and k unchanged by them, and the predicted
errors against the scatter of independent batches."""
import numpy as np
import pytest
import torch

from tests import cases, engine_cases

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-12          # moments of one correlate launch against torch sums of the terms it exported
RUN_TOL = 1e-9            # run() on its route against step(): the existing correlation tolerance (1e-8 for WM)


def _six(cq, kq):
    out = []
    for t in (cq, kq):
        out += [torch.sum(t.real * t.real), torch.sum(t.imag * t.imag), torch.sum(t.real * t.imag)]
    return torch.stack(out)


def _close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.maximum(np.abs(b), np.abs(b).max(axis=0, keepdims=True) * 1e-6 + 1e-300)
    assert np.all(np.abs(a - b) <= tol * scale), float(np.max(np.abs(a - b) / scale))


def _reference_moments(name, nt, setup=None):
    """the six sums per step from the per-trajectory terms of step() + ic_correlation(): one correlate launch per step, its own
    moments checked against the terms it exported"""
    g = cases.load(name)
    prop, pot = engine_cases.engine_propagator(g), engine_cases.engine_potential(g)
    if setup:
        setup(prop)
    dt = float(g["dt"])
    rows = []
    for _ in range(nt):
        prop.ic_correlation(pot)
        mom = torch.zeros(6, dtype=torch.float64, device=prop.device)
        slot = torch.zeros(5, dtype=torch.float64, device=prop.device)
        prop._launch_correlate(prop._rows.single(slot, mom))
        want = _six(prop._cq, prop._kq)
        _close(mom.cpu().numpy(), want.cpu().numpy(), STEP_TOL)
        rows.append(want.cpu().numpy())
        prop.step(pot, dt)
    return np.array(rows)


def _spy(monkeypatch, names):
    """count the calls of the named C-ABI entry points made by the propagators module"""
    from semiclassical_amd import propagators as PR
    real, seen = PR.lib, {}

    class Lib(object):
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in names:
                return fn

            def counted(*a):
                seen[name] = seen.get(name, 0) + 1
                return fn(*a)
            return counted
    monkeypatch.setattr(PR, "lib", Lib())
    return seen


def _no_whole_loop(prop):
    prop._whole_loop_ok = False


def _no_pairs(prop):
    prop.pair_steps = False


# name, fixture, nt, propagator set-up, run() keywords, entry point that must have run, tolerance against step()
ROUTES = [
    ("whole-loop-sep16", "hk_as5_chi002", 40, None, {}, "sc_hk_run_m", RUN_TOL),
    ("whole-loop-lin-chunks", "hk_methylium", 520, None, {}, "sc_hk_run_modal_m", 1e-8),
    ("whole-loop-lin-plain", "hk_methylium", 12, None, {}, "sc_hk_run_m", RUN_TOL),
    ("separable-step", "hk_as5_chi002", 30, _no_whole_loop, {}, "sc_hk_correlate_m", RUN_TOL),
    ("graph", "hk_as5_chi002", 30, _no_whole_loop, {"use_graph": True}, "sc_reduce_slot_moments_at", RUN_TOL),
    ("pairs", "hk_as60", 20, None, {}, "sc_hk_step_multi", RUN_TOL),
    ("tiled-single", "hk_as60", 20, _no_pairs, {}, "sc_hk_correlate_m", RUN_TOL),
    ("modal-step", "hk_coumarin_harmonic", 6, None, {}, "sc_hk_step_modal", RUN_TOL),
    ("wm-register", "wm_as5_chi002", 30, None, {}, "sc_term_moments", 1e-8),
    ("wm-methylium", "wm_methylium", 10, None, {}, "sc_term_moments", 1e-8),
]


@pytest.mark.parametrize("name,fixture,nt,setup,kw,entry,tol", ROUTES, ids=[r[0] for r in ROUTES])
def test_moments_on_every_route(monkeypatch, name, fixture, nt, setup, kw, entry, tol):
    g = cases.load(fixture)
    pot, dt = engine_cases.engine_potential(g), float(g["dt"])
    runs = []
    for with_moments in (True, False):
        prop = engine_cases.engine_propagator(g)
        if setup:
            setup(prop)
        prop._remember_nac(pot)
        slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
        moments = torch.zeros((nt, 6), dtype=torch.float64, device=prop.device) if with_moments else None
        seen = _spy(monkeypatch, {entry}) if with_moments else {}
        prop.run(pot, dt, nt, slots=slots, moments=moments, **kw)
        prop.synchronize()
        monkeypatch.undo()
        if with_moments:
            assert seen.get(entry, 0) > 0, f"{entry} was not called"
        runs.append((slots.cpu().numpy(), None if moments is None else moments.cpu().numpy()))
    assert np.array_equal(runs[0][0][:, :4], runs[1][0][:, :4]), "C or k changed with moments on"
    want = _reference_moments(fixture, nt, setup)
    _close(runs[0][1], want, tol)


def test_standard_errors_api_matches_finalize():
    """run(standard_errors=True) against finalize_moments of the raw buffers and against standard_errors() step by step"""
    g = cases.load("hk_as5_chi002")
    pot, dt, nt, E0 = engine_cases.engine_potential(g), float(g["dt"]), 8, float(g["E0"])
    a = engine_cases.engine_propagator(g)
    a._whole_loop_ok = False
    C, k, sC, sk = a.run(pot, dt, nt, energy0_es=E0, standard_errors=True)
    # at t = 0 every trajectory's C term is 1: no spread in Re C there
    assert np.isfinite(sC).all() and np.isfinite(sk).all() and (sC.real[1:] > 0).all() and (sk.real > 0).all()
    b = engine_cases.engine_propagator(g)
    b._whole_loop_ok = False
    for i in range(nt):
        b.ic_correlation(pot)
        ec, ek = b.standard_errors(E0)
        assert abs(ec - sC[i]) <= 1e-10 * abs(sC[i]) and abs(ek - sk[i]) <= 1e-10 * abs(sk[i])
        b.step(pot, dt)
    plain = engine_cases.engine_propagator(g)
    plain._whole_loop_ok = False
    c0, k0 = plain.run(pot, dt, nt, energy0_es=E0)
    assert np.array_equal(c0, C) and np.array_equal(k0, k)


@pytest.mark.parametrize("wm", [False, True], ids=["hk_as5_chi002", "wm_as5_chi002"])
def test_predicted_errors_match_the_scatter_of_independent_batches(wm):
    """64 device-sampled batches (seed fixed, subsequences 0..63) of 512 trajectories: the standard deviation of the batch means
    against the mean predicted sigma, for Re and Im of C and k at several steps"""
    from semiclassical_amd import propagators as PR
    g = cases.load("wm_as5_chi002" if wm else "hk_as5_chi002")
    pot, dt = engine_cases.engine_potential(g), float(g["dt"])
    Gi, Gt = cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"])
    nt, nb, n = 100, 64, 512
    means, sigmas = [], []
    for b in range(nb):
        prop = (PR.WaltonManolopoulosPropagator(Gi, Gt, float(g["alpha"]), float(g["beta"])) if wm else PR.HermanKlukPropagator(Gi, Gt))
        prop.initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), ntraj=n, seed=1234, subsequence=b)
        C, k, sC, sk = prop.run(pot, dt, nt, standard_errors=True)
        means.append(np.stack((C, k)))
        sigmas.append(np.stack((sC, sk)))
    means, sigmas = np.array(means), np.array(sigmas)
    for step in (5, nt // 2, nt - 1):
        for q in range(2):
            for part in (np.real, np.imag):
                emp = np.std(part(means[:, q, step]), ddof=1)
                pred = np.mean(part(sigmas[:, q, step]))
                assert 0.7 <= emp / pred <= 1.3, (step, q, emp, pred)


def test_driver_batches_fold_to_one_pooled_error(tmp_path):
    """three batches of unequal size through the driver (propagate_batch + CorrelationStore) against one batch of the same
    trajectories: pooled means, second moments and standard errors"""
    from semiclassical_amd import driver as DR
    from semiclassical_amd import hostmath
    g = cases.load("hk_as5_chi002")
    pot, dt, nt = engine_cases.engine_potential(g), float(g["dt"]), 10
    setup = DR.ProblemSetup(pot, None, None, None, float(g["E0"]), np.nan)
    times = np.arange(nt) * dt
    n = g["probi"].shape[0]
    path = str(tmp_path / "c.npz")
    np.savez(path, propagator="HK", times=times, autocorrelation=np.zeros(nt, complex), ic_correlation=np.zeros(nt, complex),
             adiabatic_gap=np.nan, zero_point_energy=0.0, trajectories=0)
    store = DR.CorrelationStore(path)
    batches = []
    for sel in (slice(0, 60), slice(60, 150), slice(150, n)):
        prop = engine_cases.engine_propagator(g, select=sel)
        batches.append((sel.stop - sel.start,) + DR.propagate_batch(prop, setup, dt, nt, times, errors=True))
    # the store asserts <phi(0)|phi(0)> ~ 1 of the pooled mean: a slice of a fixture need not meet it at step 0, so the
    # first row is set to 1 in every batch (its moments stay) and left out of the comparison
    for m, C, k, mC, mk in batches:
        C = C.copy()
        C[0] = 1.0
        store.add_batch(C, k, m, second_moments=(mC, mk))
    one = engine_cases.engine_propagator(g)
    C, k, mC, mk = DR.propagate_batch(one, setup, dt, nt, times, errors=True)
    got = np.load(path)
    assert int(got["trajectories"]) == n
    assert cases.rel_err(got["autocorrelation"][1:], C[1:]) < 1e-12 and cases.rel_err(got["ic_correlation"], k) < 1e-12
    _close(got["autocorrelation_second_moment"], mC, 1e-12)
    _close(got["ic_correlation_second_moment"], mk, 1e-12)
    _close(np.abs(got["autocorrelation_error"][1:]), np.abs(hostmath.standard_errors(C, mC / n, n))[1:], 1e-10)
    _close(np.abs(got["ic_correlation_error"]), np.abs(hostmath.standard_errors(k, mk / n, n)), 1e-10)
