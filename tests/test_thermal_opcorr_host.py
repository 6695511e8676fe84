"""Thermal operator correlation functions Tr[rho e^{iH_es t} A e^{-iH_gs t} B] with linear operators, host
side (no GPU): the restatement of tests/thermal_opcorr_cases.py -- the reference of tests/test_thermal_opcorr_gpu.py -- against
exact traces in a Fock basis and the closed form at t = 0, the folded vectors the kernels take against the direct formula, the
zero-temperature limit, the result file's pooling, the rates task on a thermal file and the C-ABI symbols."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import cases, thermal_cases as tcs, thermal_opcorr_cases as toc
from tests.test_opcorr_host import (ZERO, _operators, _record, _store, bra_factors, ket_factors, position_element, project)

torch.set_default_dtype(torch.float64)
hbar = tcs.hbar


# ------------------------------------------------------------------------------------------- 1. exactness on the 2-D model

NT, DT, NTRAJ, SEED = 30, 0.1, 20000, 7


def _model_constants(m):
    """(omega, L) of the model's initial surface as ThermalConstants orders them"""
    from semiclassical_amd import hostmath
    tc = hostmath.ThermalConstants(torch.from_numpy(m["Gamma_0"]), torch.from_numpy(m["masses"]), m["kT"])
    return tc, tc.omega.numpy(), tc.L.numpy()


@functools.lru_cache(maxsize=None)
def _exact(nbasis):
    from semiclassical_amd import hostmath
    m = tcs.model_2d()
    tc, omega, L = _model_constants(m)
    times = hostmath.time_grid(NT, DT)
    bra, ket = toc.exactness_pairs()
    # (H_es carries its zero-point energy E0: the trace is the estimate WITH the phase e^{i E0 t / hbar})
    return toc.exact_operator_traces(omega, L, m["masses"], m["q0"], m["pos_gs"], m["hess_gs"], m["kT"], times, nbasis, bra, ket)


@functools.lru_cache(maxsize=None)
def _restatements():
    m = tcs.model_2d()
    prop, pot, tc, centres = tcs.model_objects(m, m["kT"], NTRAJ, SEED)
    bra, ket = toc.exactness_pairs()
    return toc.run_restatement(prop, pot, tc, centres, DT, NT, bra, ket, m["E0"], frozen=(False, True))


def _restated(frozen_bra):
    """(X, sigma) of the estimator, or of the one whose bra centre stays at t = 0; both from one pass over the trajectories"""
    return _restatements()[frozen_bra]


def _sigmas_off(X, sigma, exact):
    """|deviation| / sigma per component, (nt, M) for Re and for Im; a component whose sigma is rounding noise carries the floor
    1e-12 |exact|"""
    floor = 1e-12 * abs(exact)
    return abs((X - exact).real) / (sigma.real + floor), abs((X - exact).imag) / (sigma.imag + floor)


def test_fock_basis_is_converged():
    change = abs(_exact((38, 32)) - _exact((48, 42))).max()
    print(f"Fock basis 38 x 32 against 48 x 42: X changes by {change:.2e}")
    assert change < 1e-10


def test_restatement_within_five_sigma_of_the_exact_traces():
    exact = _exact((38, 32))
    X, sigma = _restated(False)
    re, im = _sigmas_off(X, sigma, exact)
    worst = np.maximum(re, im).max(0)
    print("max sigma per pair:", ", ".join(f"{v:.1e}" for v in np.maximum(sigma.real, sigma.imag).max(0)),
          " largest deviation / sigma per pair:", np.array2string(worst, precision=2))
    assert max(sigma.real.max(), sigma.imag.max()) <= 0.01
    assert (re <= 5.0).all() and (im <= 5.0).all()


def test_a_frozen_bra_centre_is_seen():
    """the power of the check above: the bra centre kept at a_i(0), b_i(0) is more than 10 sigma off on each non-trivial pair"""
    exact = _exact((38, 32))
    X, sigma = _restated(True)
    re, im = _sigmas_off(X, sigma, exact)
    worst = np.maximum(re, im).max(0)
    print("frozen bra centre, largest deviation / sigma per pair:", np.array2string(worst, precision=1),
          " absolute:", np.array2string(abs(X - exact).max(0), precision=3))
    assert (worst[1:] > 10.0).all()


# ------------------------------------------------------------------------------------------- 2. closed form at t = 0

def test_closed_form_is_the_exact_trace_at_t0():
    m = tcs.model_2d()
    tc, _, _ = _model_constants(m)
    bra, ket = toc.exactness_pairs()
    closed = toc.closed_form_t0(bra, ket, m["q0"], tc)
    exact = _exact((38, 32))[0]
    print(f"closed form at t = 0 against the exact trace: {abs(closed - exact).max():.2e}")
    assert abs(closed - exact).max() <= 1e-10


def _dense_pairs(m, rng, M=3):
    D = m["q0"].shape[0]
    return (rng.normal(size=M), rng.normal(size=(M, D))), (rng.normal(size=M), rng.normal(size=(M, D)))


@pytest.mark.parametrize("model", ["2d", "dense6"])
def test_restatement_within_five_sigma_of_the_closed_form(model):
    if model == "2d":
        m, (bra, ket) = tcs.model_2d(), toc.exactness_pairs()
        X, sigma = (a[0] for a in _restated(False))
        tc = _model_constants(m)[0]
    else:
        m = tcs.synthetic_dense(6, 3)
        prop, pot, tc, centres = tcs.model_objects(m, m["kT"], 4000, 3)
        bra, ket = _dense_pairs(m, np.random.default_rng(11))
        X, sigma = toc.estimate(toc.thermal_opcorr_terms(prop, tc, centres, 0.0, bra, ket))
    closed = toc.closed_form_t0(bra, ket, m["q0"], tc)
    re, im = _sigmas_off(X, sigma, closed)
    print(f"{model}: X(0) {np.array2string(X, precision=4)}, closed form {np.array2string(closed, precision=4)}, deviation / sigma "
          f"{np.array2string(np.maximum(re, im), precision=2)}")
    assert (re <= 5.0).all() and (im <= 5.0).all()


# ------------------------------------------------------------------------------------------- 3. folded against direct

def _folded_deviation(Gi, Gt, G0, q0, masses, kT, rng, bra, ket, t=0.7, n=9):
    """largest deviation, over both sides, of  kappa + u.Q + i w.P + ut.Qc(t) + i wt.Pc(t)  (hostmath.fold_thermal_linear_operators)
    from the direct matrix element with the centre's Cartesian image, relative to max(1, |f|); random points and centres"""
    from semiclassical_amd import hostmath
    T = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    tc = hostmath.ThermalConstants(T(G0), T(masses), kT)
    D, dm = tc.dim, tc.dmodes
    centres = T(rng.normal(0.0, 0.7, (n, 2 * dm)))
    z = rng.normal(0.0, 0.8, (2 * D, n))
    worst = 0.0
    for is_ket, G, (c, m), time in ((False, Gt, bra, t), (True, Gi, ket, 0.0)):
        u, w, kap, ut, wt = (a.numpy() for a in hostmath.fold_thermal_linear_operators(T(c), T(m), T(G), T(G0), T(q0), tc, ket=is_ket))
        assert u.shape == w.shape == m.shape and ut.shape == wt.shape == (m.shape[0], dm) and kap.dtype == np.complex128
        Qc, Pc, _ = (a.numpy() for a in tcs.rotated(tc, centres, time))
        folded = kap[None, :] + (u @ z[:D]).T + 1j * (w @ z[D:]).T + (ut @ Qc).T + 1j * (wt @ Pc).T
        a, b = q0[:, None] + tc.map_q.numpy() @ Qc, tc.map_p.numpy() @ Pc
        x = position_element(z[:D], z[D:], G, a, b, G0) if is_ket else position_element(a, b, G0, z[:D], z[D:], G)
        direct = c[None, :] + (m @ x).T
        worst = max(worst, (abs(folded - direct) / np.maximum(1.0, abs(direct))).max())
    return worst, tc


def _random_pairs(rng, M, D, Gi, Gt, G0):
    return ((rng.normal(size=M), project(rng.normal(size=(M, D)), G0, Gt)), (rng.normal(size=M), project(rng.normal(size=(M, D)), Gi, G0)))


@pytest.mark.parametrize("case", ["2d", "dense6", "methylium", "diagonal"])
def test_folded_vectors_match_the_direct_formula(case):
    rng = np.random.default_rng(len(case))
    if case in ("2d", "dense6"):
        m = tcs.model_2d() if case == "2d" else tcs.synthetic_dense(6, 3)
        Gi = Gt = G0 = m["Gamma_0"]
        q0, masses, kT = m["q0"], m["masses"], m["kT"]
    elif case == "methylium":
        g = cases.load("hk_methylium")
        Gi, Gt, G0, q0 = g["Gamma_i"], g["Gamma_t"], g["Gamma_0"], g["q0"]
        masses, kT = cases.oracle_potential(g).masses().numpy().astype(np.float64), 0.004
    else:
        masses = np.array([1.0, 3.0, 0.5, 2.0])
        G0 = np.diag(np.array([0.5, 1.0, 2.2, 1.4]) * masses)
        Gi, Gt, q0, kT = G0 * 1.3, G0 * 0.8, np.array([0.2, -0.1, 0.4, 0.0]), 0.9
    D = q0.shape[0]
    bra, ket = _random_pairs(rng, 4, D, Gi, Gt, G0)
    dev, tc = _folded_deviation(Gi, Gt, G0, q0, masses, kT, rng, bra, ket)
    print(f"{case}: D = {D}, d'' = {tc.dmodes}, diag = {tc.diag}: folded against direct {dev:.2e}")
    assert tc.diag == (case == "diagonal") and (tc.dmodes < D) == (case == "methylium")
    assert dev <= 1e-12


def test_vector_outside_the_range_is_refused():
    from semiclassical_amd import hostmath
    g = cases.load("hk_methylium")
    T = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    Gt, G0 = g["Gamma_t"], g["Gamma_0"]
    D = Gt.shape[0]
    tc = hostmath.ThermalConstants(T(G0), cases.oracle_potential(g).masses().to(torch.float64), 0.004)
    e, V = np.linalg.eigh(Gt + G0)
    null = V[:, abs(e) <= ZERO][:, 0]
    inside = project(np.random.default_rng(1).normal(size=(2, D)), Gt, G0)
    args = (T(Gt), T(G0), T(g["q0"]), tc)
    hostmath.fold_thermal_linear_operators(T(np.zeros(2)), T(inside), *args, ket=False)
    for ket in (False, True):
        with pytest.raises(ValueError, match=r"\[1\]"):
            hostmath.fold_thermal_linear_operators(
                T(np.zeros(2)), T(np.vstack((inside[0], inside[1] + 1e-6 * np.linalg.norm(inside[1]) * null))), *args, ket=ket)


# ------------------------------------------------------------------------------------------- 4. zero temperature

def test_zero_temperature_is_the_operator_correlation_of_phi0():
    """at k_B T = 0 every centre is (q0, 0): the terms are those of the zero-temperature restatement (tests/test_opcorr_host.py)"""
    m = tcs.model_2d()
    prop, pot, tc, centres = tcs.model_objects(m, 0.0, 200, 5)
    assert not centres.any()
    bra, ket = toc.exactness_pairs()
    worst = 0.0
    for _ in range(3):
        prop.step(pot, DT)
        x = toc.thermal_opcorr_terms(prop, tc, centres, prop.t, bra, ket)
        cq = tcs.thermal_terms(prop, tc, centres, prop.t)[0].numpy()
        (q, p), (Q, P) = ((a.numpy() for a in pair) for pair in (prop.initial_positions_and_momenta(), prop.current_positions_and_momenta()))
        G0, q0, p0 = m["Gamma_0"], m["q0"], np.zeros(2)
        cold = bra_factors(bra[0], bra[1], Q, P, G0, G0, q0, p0) * ket_factors(ket[0], ket[1], q, p, G0, G0, q0, p0) * cq[:, None]
        worst = max(worst, abs(x - cold).max() / abs(cold).max())
    print(f"k_B T = 0 against the zero-temperature restatement: {worst:.2e}")
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------- 5. the result file and the rates task

def test_store_pools_thermal_operator_batches(tmp_path):
    from semiclassical_amd import driver, hostmath
    rng = np.random.default_rng(4)
    nt, M, D, n1, n2, kelvin = 3, 2, 2, 30, 50, 300.0
    ops = _operators(rng, M, D)
    a1, r1, x1 = _record(rng, nt, ops, n1)
    a2, r2, x2 = _record(rng, nt, ops, n2)
    store = _store(tmp_path, "thermal.npz", nt)
    store.add_batch(a1, a1, n1, operators=r1, temperature=kelvin)
    store.add_batch(a2, a2, n2, operators=r2, temperature=kelvin)
    got = dict(np.load(store.path))
    n = n1 + n2
    x = np.concatenate((n1 * x1, n2 * x2), axis=2) / n
    assert float(got["temperature"]) == kelvin and int(got["trajectories"]) == n
    assert all(np.array_equal(got["operator_" + key], ops[key]) for key in ops)
    assert np.allclose(got["operator_correlation"], x.sum(2), rtol=1e-13, atol=0)
    m3 = np.stack(((x.real ** 2).sum(2), (x.imag ** 2).sum(2), (x.real * x.imag).sum(2)), axis=2)
    assert np.allclose(got["operator_correlation_error"], hostmath.standard_errors(x.sum(2), m3, n), rtol=1e-10, atol=0)
    # other operators, another temperature or none: refused, and the file stays as it was
    before = dict(np.load(store.path))
    for kw in (dict(operators=dict(r2, bra_c=ops["bra_c"] + 1e-9), temperature=kelvin), dict(operators=r2, temperature=250.0),
               dict(operators=r2), dict(temperature=kelvin)):
        with pytest.raises(driver.ConfigurationError):
            store.add_batch(a2, a2, n2, **kw)
    after = dict(np.load(store.path))
    assert set(before) == set(after) and all(np.array_equal(before[k], after[k]) for k in before)
    task = {"results": {"overwrite": False}}
    same = tuple(ops[key] for key in ("bra_c", "bra_m", "ket_c", "ket_m"))
    times = torch.linspace(0.0, 1.0, nt)
    for kw in (dict(operators=(same[0] + 1.0,) + same[1:], temperature=kelvin), dict(operators=same), dict(temperature=kelvin)):
        with pytest.raises(driver.ConfigurationError):
            store.start(task, "HK", times, None, **kw)
    store.start(task, "HK", times, None, operators=same, temperature=kelvin)


def test_rates_task_on_a_thermal_file(tmp_path):
    """the rates task needs no change: a file with ``temperature`` and operator correlation functions gains operator_lineshape and
    radiative_rate, computed by rates.lineshape_from_correlation and rates.radiative_rate"""
    from semiclassical_amd import driver, rates, units
    rng = np.random.default_rng(12)
    nt, M = 32, 2
    times = np.linspace(0.0, 400.0, nt)
    k = (rng.normal(size=nt) + 1j * rng.normal(size=nt)) * np.exp(-times / 90.0)
    X = (rng.normal(size=(nt, M)) + 1j * rng.normal(size=(nt, M))) * np.exp(-times / 90.0)[:, None]
    np.savez(tmp_path / "thermal.npz", propagator="HK", times=times, autocorrelation=k, ic_correlation=k, trajectories=10,
             temperature=300.0, operator_correlation=X)
    driver.calculate_rates({"correlations": str(tmp_path / "thermal.npz"), "rates": str(tmp_path / "rates.npz"), "adiabatic_gap_ev": 3.0})
    out = dict(np.load(tmp_path / "rates.npz"))
    lineshape, _ = driver.lineshape_from_task({})
    energies, G = rates.lineshape_from_correlation(times, X[:, 1], lineshape)
    assert np.array_equal(out["operator_lineshape"][:, 1], G[energies >= 0.0].real)
    assert float(out["radiative_rate"]) == rates.radiative_rate(out["energies"], out["operator_lineshape"].sum(1), 3.0 / units.hartree_to_ev)
    assert float(out["temperature"]) == 300.0


def test_driver_refusals_without_a_device(tmp_path):
    """WM with the key is refused whatever the temperature, before a device is touched"""
    from semiclassical_amd import driver
    task = {"task": "dynamics", "propagator": "WM", "operator_correlation": str(tmp_path / "t.npz"), "temperature": 300.0,
            "potential": {"type": "none"}}
    with pytest.raises(driver.ConfigurationError, match="WM"):
        driver.run_semiclassical_dynamics(task)


# ------------------------------------------------------------------------------------------- 6. interface and ABI

def test_propagators_offer_thermal_operator_correlation():
    import inspect
    from semiclassical_amd import hostmath, propagators as PR
    sig = inspect.signature(PR.HermanKlukPropagator.thermal_operator_correlation).parameters
    assert list(sig)[1:] == ["bra", "ket", "energy0_es", "standard_errors"] and sig["ket"].default is None
    run = inspect.signature(PR.HermanKlukPropagator.run).parameters
    assert list(run)[-2:] == ["thermal_operators", "thermal_opcorr"] and run["thermal_operators"].default is None
    assert [f.arg for f in PR._ROW_FAMILIES] == ["targets", "operators", "thermal_operators"]
    assert callable(hostmath.fold_thermal_linear_operators)
    assert PR.WaltonManolopoulosPropagator._opcorr_ok is False


def test_symbols_are_declared_bound_and_exported():
    from semiclassical_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "semiclassical_hip.h")).read()
    for name in ("sc_hk_opcorr_thermal", "sc_hk_opcorr_thermal_initial", "sc_hk_opcorr_thermal_rows"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib.sc_abi_version() == 18
    rows = _lib.lib.sc_hk_opcorr_thermal_rows
    assert rows(1, 1) == 1 and rows(64, 500) == 1 and rows(65, 1) == 2 and rows(130, 65) == 3 and rows(0, 5) == 0
