"""Time-averaged Herman-Kluk spectra, host side (no GPU): the numpy restatement of the definitions
(tests/timeavg_cases.py) against the closed form of the harmonic oscillator and against Parseval's identity, then the host
pieces: finalize_time_average, the result file's pooling and refusals, the C-ABI symbols."""
import os
import re

import numpy as np
import pytest

from tests import timeavg_cases as ta
from tests.test_cross_host import _store


# ------------------------------------------------------------------------------------------- 1. the oscillator

@pytest.fixture(scope="module")
def oscillator():
    N = ta.OSC["N"]
    q, p, prob = ta.oscillator_sample(N)
    g = ta.oscillator_terms(q, p)
    return g, prob, N


def test_restatement_meets_the_closed_form(oscillator):
    """1-D harmonic oscillator, omega = gamma = 1, q0 = 1.6, dt = 0.05, ns = 2000, N = 2048 points of the Husimi density of chi
    on analytic trajectories: within 5 sigma of the closed form at the six energies, sigma / I <= 0.3 at the three peaks"""
    g, prob, N = oscillator
    I, sigma = ta.restated_spectrum(g, ta.OSC_ENERGIES, 0.0, ta.OSC["dt"], N * 2.0 * np.pi, prob, N)
    exact = ta.oscillator_closed_form(ta.OSC_ENERGIES)
    for e, E in enumerate(ta.OSC_ENERGIES):
        print(f"E = {E}: I {I[0, e]:.5f}  closed form {exact[e]:.5f}  sigma {sigma[0, e]:.2e}  |dev| / sigma "
              f"{abs(I[0, e] - exact[e]) / sigma[0, e]:.2f}  sigma / I {sigma[0, e] / I[0, e]:.3f}")
    assert abs(exact[0] - np.exp(-1.28) * 100.0 / (2.0 * np.pi)) < 0.01 * exact[0]          # the peak at E = 1/2: P_0 T / 2 pi = 4.43
    assert (I >= 0).all()
    assert (abs(I[0] - exact) <= 5.0 * sigma[0]).all()
    assert (sigma[0, list(ta.OSC_PEAKS)] / I[0, list(ta.OSC_PEAKS)] <= 0.3).all()


def test_every_trajectory_adds_a_non_negative_number(oscillator):
    g, prob, N = oscillator
    A = ta.restated_accumulator(g[:200, :16], ta.OSC_ENERGIES, 0.0, ta.OSC["dt"])
    I, S2 = ta.restated_sums(A, 200 * ta.OSC["dt"], N * 2.0 * np.pi, prob[:16])
    one, _ = ta.restated_sums(A[3:4], 200 * ta.OSC["dt"], N * 2.0 * np.pi, prob[3:4])
    assert (one >= 0).all() and (I >= one).all() and (S2 >= one ** 2 * (1 - 1e-14)).all()


# ------------------------------------------------------------------------------------------- 2. Parseval

def test_parseval():
    """NE = ns, E_e = 2 pi hbar e / (ns dt):  sum_e I(E_e) 2 pi hbar / (ns dt) = 1/ns sum_s sum_i |g_i(t_s)|^2 / (mc_norm P_i)"""
    rng = np.random.default_rng(3)
    ns, n, K, dt, t_a, mc_norm = 24, 11, 3, 0.3, 1.7, 40.0
    g = rng.normal(size=(ns, n, K)) + 1j * rng.normal(size=(ns, n, K))
    probi = rng.uniform(0.5, 1.5, n)
    energies = 2.0 * np.pi * ta.HBAR * np.arange(ns) / (ns * dt)
    I, _ = ta.restated_sums(ta.restated_accumulator(g, energies, t_a, dt), ns * dt, mc_norm, probi)
    left = I.sum(1) * 2.0 * np.pi * ta.HBAR / (ns * dt)
    right = (np.abs(g) ** 2 / (mc_norm * probi[None, :, None])).sum((0, 1)) / ns
    print(f"Parseval: {abs(left - right).max() / abs(right).max():.2e}")
    assert abs(left - right).max() <= 1e-12 * abs(right).max()


# ------------------------------------------------------------------------------------------- 3. host pieces

def _raw(rng, K, NE, n, T):
    """raw sums (K, NE, 2) of a batch of n samples: y T and (y T)^2 with the weight 1 / n inside y"""
    y = rng.uniform(0.0, 2.0, (n, K, NE)) / n
    return np.stack(((y * T).sum(0), ((y * T) ** 2).sum(0)), axis=2), y


def test_finalize_time_average():
    from semiclassical_amd.propagators import HermanKlukPropagator as HK
    rng = np.random.default_rng(5)
    K, NE, n, T = 2, 5, 40, 3.5
    raw, y = _raw(rng, K, NE, n, T)
    I, sigma = HK.finalize_time_average(raw, T, n)
    assert I.shape == sigma.shape == (K, NE) and I.dtype == sigma.dtype == np.float64
    assert np.allclose(I, y.sum(0), rtol=1e-13, atol=0)
    # the standard error of the mean of the n samples n y: sqrt(var / n), with the unbiased variance
    assert np.allclose(sigma, np.sqrt(np.var(n * y, axis=0, ddof=1) / n), rtol=1e-10, atol=0)
    # the buffers of two ranks that share one ensemble add
    half = _raw(rng, K, NE, n, T)[0]
    both, _ = HK.finalize_time_average(raw + half, T, 2 * n)
    assert np.allclose(both, I + half[..., 0] / T, rtol=1e-13, atol=0)


def _record(rng, K, NE, n, T, energies, Q, P, errors=True):
    raw, y = _raw(rng, K, NE, n, T)
    rec = {"energies": energies, "q": Q, "p": P, "window": T, "spectrum": raw[..., 0] / T}
    if errors:
        rec["second_moment"] = n * raw[..., 1] / T ** 2
    return rec, y


def test_store_pools_batches(tmp_path):
    """two batches pooled equal one batch of both: the mean with the weights of the autocorrelation, the error from the pooled
    second moment"""
    rng = np.random.default_rng(7)
    nt, K, NE, D, n1, n2, T = 3, 2, 4, 2, 30, 50, 2.5
    energies, Q, P = rng.normal(size=NE), rng.normal(size=(K, D)), rng.normal(size=(K, D))
    r1, y1 = _record(rng, K, NE, n1, T, energies, Q, P)
    r2, y2 = _record(rng, K, NE, n2, T, energies, Q, P)
    a = np.ones(nt, dtype=complex)
    store = _store(tmp_path, "two.npz", nt)
    store.add_batch(a, a, n1, time_average=r1)
    store.add_batch(a, a, n2, time_average=r2)
    got = dict(np.load(store.path))
    n = n1 + n2
    y = np.concatenate((n1 * y1, n2 * y2)) / n               # the same samples as ONE batch with the weight 1 / (n1 + n2)
    assert np.array_equal(got["ta_energies"], energies) and np.array_equal(got["ta_references_q"], Q)
    assert np.array_equal(got["ta_references_p"], P) and float(got["ta_window"]) == T
    assert np.allclose(got["ta_spectrum"], y.sum(0), rtol=1e-13, atol=0)
    assert np.allclose(got["ta_spectrum_second_moment"], n * (y ** 2).sum(0), rtol=1e-12, atol=0)
    assert np.allclose(got["ta_spectrum_error"], ta.standard_error(y.sum(0), (y ** 2).sum(0), n), rtol=1e-10, atol=0)
    assert int(got["trajectories"]) == n
    # a batch without second moments: the spectrum pools on, the error keys go
    r3, _ = _record(rng, K, NE, n1, T, energies, Q, P, errors=False)
    store.add_batch(a, a, n1, time_average=r3)
    got = np.load(store.path)
    assert "ta_spectrum" in got and "ta_spectrum_error" not in got and "ta_spectrum_second_moment" not in got


def test_store_refuses_other_energies(tmp_path):
    import torch
    from semiclassical_amd import driver
    rng = np.random.default_rng(9)
    nt, K, NE, D, T = 3, 2, 4, 2, 2.5
    energies, Q, P = rng.normal(size=NE), rng.normal(size=(K, D)), rng.normal(size=(K, D))
    rec, _ = _record(rng, K, NE, 20, T, energies, Q, P)
    a = np.ones(nt, dtype=complex)
    store = _store(tmp_path, "other.npz", nt)
    store.add_batch(a, a, 20, time_average=rec)
    before = dict(np.load(store.path))
    for other in (dict(rec, energies=energies + 1e-9), dict(rec, energies=energies[:3], spectrum=rec["spectrum"][:, :3]),
                  dict(rec, q=Q[::-1].copy()), dict(rec, p=P + 1.0), dict(rec, window=T + 0.1), None):
        with pytest.raises(driver.ConfigurationError):
            store.add_batch(a, a, 20, time_average=other)
    plain = _store(tmp_path, "plain.npz", nt)
    plain.add_batch(a, a, 20)
    with pytest.raises(driver.ConfigurationError):
        plain.add_batch(a, a, 20, time_average=rec)
    after = dict(np.load(store.path))
    assert set(before) == set(after) and all(np.array_equal(before[k], after[k]) for k in before)
    # start() refuses before any trajectory runs
    task, times = {"results": {"overwrite": False}}, torch.linspace(0.0, 1.0, nt)
    for idents in ((energies + 1.0, Q, P, T), (energies, Q, P, 2 * T), None):
        with pytest.raises(driver.ConfigurationError):
            store.start(task, "HK", times, None, time_average=idents)
    store.start(task, "HK", times, None, time_average=(energies, Q, P, T))


def test_store_without_the_key_has_todays_keys(tmp_path):
    store = _store(tmp_path, "none.npz", 3)
    a = np.ones(3, dtype=complex)
    store.add_batch(a, a, 10)
    assert set(np.load(store.path).keys()) == {"propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap",
                                               "zero_point_energy", "trajectories"}


def test_driver_refuses_wm_and_bad_files(tmp_path):
    import torch
    from collections import namedtuple
    from semiclassical_amd import driver
    task = {"task": "dynamics", "propagator": "WM", "time_averaged_spectrum": str(tmp_path / "t.npz"), "potential": {"type": "none"}}
    with pytest.raises(driver.ConfigurationError, match="WM"):
        driver.run_semiclassical_dynamics(task)
    setup = namedtuple("S", "q0 p0")(torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64))
    np.savez(tmp_path / "t.npz", energies=np.array([0.1, 0.2]))
    E, q, p = driver._load_time_average(str(tmp_path / "t.npz"), setup)
    assert np.array_equal(E, [0.1, 0.2]) and np.array_equal(q, np.zeros((1, 3))) and np.array_equal(p, np.ones((1, 3)))
    for name, arrays in (("a", dict(q=np.zeros((2, 3)), p=np.zeros((2, 3)))), ("b", dict(energies=np.zeros(0))),
                         ("c", dict(energies=np.array([np.nan]))), ("d", dict(energies=np.ones(2), q=np.zeros((2, 3)))),
                         ("e", dict(energies=np.ones(2), q=np.zeros((2, 4)), p=np.zeros((2, 4)))),
                         ("f", dict(energies=np.ones(2), q=np.zeros((65, 3)), p=np.zeros((65, 3))))):
        np.savez(tmp_path / (name + ".npz"), **arrays)
        with pytest.raises(driver.ConfigurationError, match="time_averaged_spectrum"):
            driver._load_time_average(str(tmp_path / (name + ".npz")), setup)


# ------------------------------------------------------------------------------------------- 4. ABI and interface

def test_symbols_are_declared_bound_and_exported():
    from semiclassical_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "semiclassical_hip.h")).read()
    for name in ("sc_hk_ta_block", "sc_hk_ta_terms", "sc_hk_ta_accumulate", "sc_hk_ta_finish_rows", "sc_hk_ta_finish"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib.sc_abi_version()
    TB = _lib.lib.sc_hk_ta_block()
    assert TB == 32
    rows = _lib.lib.sc_hk_ta_finish_rows
    assert [rows(n) for n in (0, 1, 64, 65, 130)] == [0, 1, 1, 2, 3]
    # refusals that need no device memory: the arguments are judged before anything is launched
    lib, dummy = _lib.lib, 4096
    assert lib.sc_hk_ta_accumulate(None, 5, 1, 1, dummy, 1, 0.0, 0.1, 0, dummy, dummy, None) == -1
    for count in (0, TB + 1):
        assert lib.sc_hk_ta_accumulate(dummy, 5, 1, count, dummy, 1, 0.0, 0.1, 0, dummy, dummy, None) == -1
        assert str(TB).encode() in lib.sc_last_error()
    assert lib.sc_hk_ta_accumulate(dummy, 5, 0, 1, dummy, 1, 0.0, 0.1, 0, dummy, dummy, None) == -1
    assert lib.sc_hk_ta_accumulate(dummy, 5, 1, 1, dummy, 0, 0.0, 0.1, 0, dummy, dummy, None) == -1
    assert lib.sc_hk_ta_accumulate(dummy, 5, 65, 1, dummy, 1, 0.0, 0.1, 0, dummy, dummy, None) == -2 and b"64" in lib.sc_last_error()
    assert lib.sc_hk_ta_accumulate(dummy, 5, 1, 1, dummy, 65536, 0.0, 0.1, 0, dummy, dummy, None) == -2 and b"65535" in lib.sc_last_error()
    assert lib.sc_hk_ta_finish(dummy, 5, 1, 65536, dummy, 1.0, None, dummy, dummy, None) == -2 and b"65535" in lib.sc_last_error()
    assert lib.sc_hk_ta_finish(dummy, 64 * 65535 + 1, 1, 1, dummy, 1.0, None, dummy, dummy, None) == -2
    assert str(64 * 65535).encode() in lib.sc_last_error()
    assert lib.sc_hk_ta_finish(dummy, 5, 1, 1, dummy, 1.0, None, None, dummy, None) == -1


def test_propagators_offer_time_averages():
    import inspect
    from semiclassical_amd import propagators as PR
    HK = PR.HermanKlukPropagator
    assert callable(HK.time_average) and callable(HK.finalize_time_average)
    run = inspect.signature(HK.run).parameters
    assert "time_average" in run and run["time_average"].default is None
    sig = inspect.signature(HK.time_average).parameters
    assert list(sig)[1:] == ["energies", "dt", "references", "max_bytes"] and sig["max_bytes"].default == 2 ** 32
    for name in ("add", "spectrum", "raw_sums"):
        assert callable(getattr(PR.TimeAverageAccumulator, name))
