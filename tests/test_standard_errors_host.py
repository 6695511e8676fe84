"""Standard errors of C_auto(t) and k_ic(t) without a GPU: the phase rotation and the sigma formula against a direct numpy
computation, CorrelationStore's folding of batches, the legacy-file and stale-key cases, the declared entry points."""
import os
import re

import numpy as np
import pytest

from semiclassical_amd import hostmath
from semiclassical_amd.units import hbar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rng = np.random.default_rng(7)


def _terms(n, nt):
    """per-trajectory terms c_i (weight 1/n inside) of nt steps, correlated Re / Im parts"""
    x = rng.normal(size=(nt, n)) + 0.3 + 1j * (0.5 * rng.normal(size=(nt, n)) + 0.2 * rng.normal(size=(nt, n)))
    return x / n


def _sums(c):
    return np.stack((np.sum(c.real ** 2, -1), np.sum(c.imag ** 2, -1), np.sum(c.real * c.imag, -1)), -1)


def _direct_sigma(c, n):
    x = n * c
    return np.std(x.real, axis=-1, ddof=1) / np.sqrt(n) + 1j * np.std(x.imag, axis=-1, ddof=1) / np.sqrt(n)


def test_rotation_and_sigma_against_direct_computation():
    import torch
    from semiclassical_amd.propagators import HermanKlukPropagator as HK
    n, nt, t0, dt, E0 = 300, 7, 2.5, 0.7, 0.013
    c, k = _terms(n, nt), _terms(n, nt)
    slots = np.zeros((nt, 5))
    slots[:, 0], slots[:, 1] = c.sum(-1).real, c.sum(-1).imag
    slots[:, 2], slots[:, 3] = k.sum(-1).real, k.sum(-1).imag
    moments = np.concatenate((_sums(c), _sums(k)), -1)
    sC, sk = HK.finalize_moments(torch.from_numpy(slots), torch.from_numpy(moments), t0, dt, E0, n)
    theta = (t0 + hostmath.time_grid(nt, dt)) * E0 / hbar
    ph = np.exp(1j * theta)[:, None]
    assert np.allclose(sC, _direct_sigma(c * ph, n), rtol=1e-12, atol=0)
    assert np.allclose(sk, _direct_sigma(k * ph, n), rtol=1e-12, atol=0)
    rot = hostmath.rotate_second_moments(_sums(c), theta)
    assert np.allclose(rot, _sums(c * ph), rtol=1e-12, atol=1e-18)


def test_single_trajectory_gives_nan():
    s = hostmath.standard_errors(np.array([0.5 + 0.5j]), np.array([[0.25, 0.25, 0.25]]), 1)
    assert np.isnan(s.real).all() and np.isnan(s.imag).all()


def _store(tmp_path, nt, errors_in_file=None):
    from semiclassical_amd import driver as DR
    path = str(tmp_path / "correlations.npz")
    np.savez(path, propagator="HK", times=np.arange(nt, dtype=float), autocorrelation=np.zeros(nt, complex),
             ic_correlation=np.zeros(nt, complex), adiabatic_gap=np.nan, zero_point_energy=0.0, trajectories=0)
    return DR.CorrelationStore(path), path


def _batch(n, nt):
    c, k = _terms(n, nt), _terms(n, nt)
    c[0] = 1.0 / n                          # <phi(0)|phi(0)> = 1, which add_batch checks
    return c, k


def _summary(c, k):
    n = c.shape[-1]
    return c.sum(-1), k.sum(-1), n, (n * _sums(c), n * _sums(k))


@pytest.mark.parametrize("sizes", [(200, 57), (31, 400, 129)])
def test_store_folds_batches_like_one_pooled_computation(tmp_path, sizes):
    nt = 5
    store, path = _store(tmp_path, nt)
    parts = [_batch(m, nt) for m in sizes]
    for c, k in parts:
        C, K, m, mom = _summary(c, k)
        store.add_batch(C, K, m, second_moments=mom)
    N = sum(sizes)
    # the pooled sample: terms of every batch re-weighted to 1/N
    call = np.concatenate([c * c.shape[-1] for c, _ in parts], -1) / N
    kall = np.concatenate([k * k.shape[-1] for _, k in parts], -1) / N
    got = np.load(path)
    assert int(got["trajectories"]) == N
    assert np.allclose(got["autocorrelation"], call.sum(-1), rtol=1e-13, atol=1e-16)
    assert np.allclose(got["autocorrelation_second_moment"], N * _sums(call), rtol=1e-13, atol=0)
    assert np.allclose(got["ic_correlation_second_moment"], N * _sums(kall), rtol=1e-13, atol=0)
    assert np.allclose(got["ic_correlation_error"], _direct_sigma(kall, N), rtol=1e-13, atol=0)
    err = got["autocorrelation_error"]
    assert np.allclose(err[1:], _direct_sigma(call, N)[1:], rtol=1e-13, atol=0)


def test_file_without_moments_drops_the_error_keys(tmp_path, caplog):
    nt = 4
    store, path = _store(tmp_path, nt)
    c, k = _batch(50, nt)
    C, K, m, mom = _summary(c, k)
    store.add_batch(C, K, m)                                    # a legacy batch: no moments
    keys = set(np.load(path).files)
    store.add_batch(C, K, m, second_moments=mom)                # errors asked for, but 50 stored trajectories have none
    assert set(np.load(path).files) == keys
    assert "standard errors dropped" in caplog.text


def test_task_without_moments_drops_stale_error_keys(tmp_path, caplog):
    nt = 4
    store, path = _store(tmp_path, nt)
    c, k = _batch(50, nt)
    C, K, m, mom = _summary(c, k)
    store.add_batch(C, K, m, second_moments=mom)
    assert "autocorrelation_error" in np.load(path).files
    store.add_batch(C, K, m)
    files = set(np.load(path).files)
    assert not files & {"autocorrelation_error", "ic_correlation_error", "autocorrelation_second_moment",
                        "ic_correlation_second_moment"}
    assert "standard errors dropped" in caplog.text


def test_default_file_has_todays_keys(tmp_path):
    nt = 3
    store, path = _store(tmp_path, nt)
    c, k = _batch(20, nt)
    C, K, m, _ = _summary(c, k)
    store.add_batch(C, K, m)
    assert sorted(np.load(path).files) == sorted(["propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap",
                                                  "zero_point_energy", "trajectories"])


def test_moment_entry_points_are_declared_and_bound():
    from semiclassical_amd import _lib
    header = open(os.path.join(ROOT, "include", "semiclassical_hip.h")).read()
    for name in ("sc_hk_correlate_m", "sc_term_moments_grid", "sc_term_moments", "sc_reduce_moments", "sc_reduce_slot_moments_at", "sc_hk_run_m",
                 "sc_hk_run_modal_m", "sc_hk_run_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 18
    assert _lib.lib.sc_hk_run_scratch_doubles(1000, 5, 10, 1) == 11 * _lib.lib.sc_hk_run_slots(1000, 5) * 10
    assert _lib.lib.sc_hk_run_scratch_doubles(1000, 5, 10, 0) == 5 * _lib.lib.sc_hk_run_slots(1000, 5) * 10
