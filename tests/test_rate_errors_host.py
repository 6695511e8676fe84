"""Error bars of the rate k_ic(E) by batch means, without a GPU: the block estimator against the per-sample standard error, its
statistical consistency on time-correlated synthetic terms, CorrelationStore's folding of the blocks, the legacy-file and
stale-key rules, the partition, and the declared entry points."""
import os
import re

import numpy as np
import pytest

from semiclassical_amd import broadening, hostmath, rates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rng = np.random.default_rng(11)


def _correlated_terms(n, nt, seed):
    """per-trajectory terms c_i(t) (weight 1/n inside), complex and strongly correlated along t: every trajectory is a damped
    oscillation with its own amplitude, frequency, phase and decay"""
    r = np.random.default_rng(seed)
    t = np.arange(nt)[:, None]
    amp = r.normal(1.0, 0.6, n) + 1j * r.normal(0.0, 0.4, n)
    om = r.normal(0.35, 0.12, n)
    gam = r.uniform(0.0, 0.05, n)
    return amp * np.exp(1j * (om * t + r.uniform(-0.3, 0.3, n)) - gam * t) / n


def _block_sums(c, B):
    """(nt, n) terms -> (nt, B) block sums and the counts, by the partition of hostmath.error_block"""
    n = c.shape[1]
    blk = hostmath.error_block(np.arange(n), B)
    sums = np.stack([c[:, blk == b].sum(axis=1) for b in range(B)], axis=1)
    return sums, np.bincount(blk, minlength=B)


def _per_sample_rate_error(times, c, lineshape):
    """exact per-sample standard error of Re rate(E): the (linear) transform of every trajectory's own estimate n c_i(t)"""
    n = c.shape[1]
    per = np.array([rates.rate_from_correlation(times, n * c[:, i], lineshape)[1].real for i in range(n)])
    return np.std(per, axis=0, ddof=1) / np.sqrt(n)


def test_partition_and_counts():
    assert list(hostmath.error_block(np.arange(12), 2)) == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]
    for n in (0, 1, 3, 4, 5, 64, 203, 400, 16503):
        for B in (2, 8, 32, 64):
            want = np.bincount(hostmath.error_block(np.arange(n), B), minlength=B) if n else np.zeros(B, dtype=int)
            assert np.array_equal(hostmath.block_counts(n, B), want), (n, B)
    for bad in (0, 1, 3, 12, 128):
        with pytest.raises(ValueError):
            hostmath.block_counts(100, bad)


def test_one_sample_per_block_is_the_per_sample_standard_error():
    n = 257
    x = rng.normal(0.3, 1.0, (n, 5)) + 1j * rng.normal(-0.2, 0.5, (n, 5))
    got = hostmath.block_standard_error(x, np.ones(n))
    want = np.std(x.real, axis=0, ddof=1) / np.sqrt(n) + 1j * np.std(x.imag, axis=0, ddof=1) / np.sqrt(n)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    got = hostmath.block_standard_error(x.real, np.ones(n))
    assert np.allclose(got, want.real, rtol=1e-12, atol=0)
    # the same through the rate: B = N blocks of one trajectory each
    nt, m = 16, 64
    c = _correlated_terms(m, nt, 3)
    times = np.arange(nt, dtype=float)
    shape = broadening.gaussian(0.1)
    _, sigma = rates.rate_standard_error(times, c, np.ones(m), shape)
    assert np.allclose(sigma, _per_sample_rate_error(times, c, shape), rtol=1e-12, atol=0)


def test_empty_blocks_are_dropped_and_one_block_gives_nan():
    v = np.array([1.0, 5.0, 2.0, 9.0])
    assert np.isclose(hostmath.block_standard_error(v, [3, 0, 5, 0]), hostmath.block_standard_error(v[[0, 2]], [3, 5]), rtol=1e-15)
    assert np.isnan(hostmath.block_standard_error(v, [4, 0, 0, 0]))
    assert np.isnan(hostmath.block_standard_error(np.array([[1.0, 2.0]]), [7])).all()
    # unequal blocks: the ANOVA form written out
    n = np.array([3.0, 5.0])
    f = np.array([1.0, 2.0])
    pooled = (n * f).sum() / 8.0
    assert np.isclose(hostmath.block_standard_error(f, n), np.sqrt((n * (f - pooled) ** 2).sum() / ((2 - 1) * 8.0)), rtol=1e-15)


def test_block_error_of_the_rate_is_consistent_with_the_per_sample_error():
    """N = 4096 time-correlated terms in B = 32 blocks: at every energy the batch-means error of the rate against the exact
    per-sample error.  The estimate has 31 degrees of freedom: relative spread 1 / sqrt(2 * 31) = 12.7 %; [0.6, 1.6] is 4.7
    sigma of it on the upper side and 3.1 on the lower"""
    n, B, nt = 4096, 32, 64
    c = _correlated_terms(n, nt, 2024)
    times = np.arange(nt, dtype=float)
    shape = broadening.gaussian(0.05)
    sums, counts = _block_sums(c, B)
    assert np.array_equal(counts, hostmath.block_counts(n, B))
    energies, sigma = rates.rate_standard_error(times, sums, counts, shape)
    want_e, rate = rates.rate_from_correlation(times, c.sum(axis=1), shape)
    assert np.array_equal(energies, want_e) and sigma.shape == rate.shape
    ratio = sigma / _per_sample_rate_error(times, c, shape)
    print("ratio of the block error to the per-sample error: min %.3f max %.3f mean %.3f" % (ratio.min(), ratio.max(), ratio.mean()))
    assert np.all(ratio >= 0.6) and np.all(ratio <= 1.6), (ratio.min(), ratio.max())


# ---------------------------------------------------------------------------------------------------------------- the store
TODAY = ["propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories"]
BLOCK_KEYS = ["autocorrelation_blocks", "ic_correlation_blocks", "block_trajectories"]


def _store(tmp_path, nt, name="correlations.npz"):
    from semiclassical_amd import driver as DR
    path = str(tmp_path / name)
    np.savez(path, propagator="HK", times=np.arange(nt, dtype=float), autocorrelation=np.zeros(nt, complex),
             ic_correlation=np.zeros(nt, complex), adiabatic_gap=np.nan, zero_point_energy=0.0, trajectories=0)
    return DR.CorrelationStore(path), path


def _batch(n, nt, seed):
    c, k = _correlated_terms(n, nt, seed), _correlated_terms(n, nt, seed + 100)
    c[0] = 1.0 / n                          # <phi(0)|phi(0)> = 1, which add_batch checks
    return c, k


def _blocks_of(c, k, B):
    cb, counts = _block_sums(c, B)
    kb, _ = _block_sums(k, B)
    return cb, kb, counts


def test_store_folds_blocks_like_one_pooled_computation(tmp_path):
    nt, B, sizes = 6, 8, (200, 57, 131)
    store, path = _store(tmp_path, nt)
    parts = [_batch(m, nt, 40 + i) for i, m in enumerate(sizes)]
    for c, k in parts:
        store.add_batch(c.sum(-1), k.sum(-1), c.shape[1], blocks=_blocks_of(c, k, B))
    N = sum(sizes)
    got = np.load(path)
    assert sorted(got.files) == sorted(TODAY + BLOCK_KEYS)
    # the pooled set: block b of the file is block b of every batch, the terms re-weighted to 1/N
    wantC = sum(_block_sums(c * c.shape[1], B)[0] for c, _ in parts) / N
    wantk = sum(_block_sums(k * k.shape[1], B)[0] for _, k in parts) / N
    counts = sum(hostmath.block_counts(m, B) for m in sizes)
    assert np.array_equal(got["block_trajectories"], counts) and int(counts.sum()) == N == int(got["trajectories"])
    assert np.allclose(got["autocorrelation_blocks"], wantC, rtol=1e-13, atol=1e-17)
    assert np.allclose(got["ic_correlation_blocks"], wantk, rtol=1e-13, atol=1e-17)
    assert np.allclose(got["autocorrelation_blocks"].sum(axis=1), got["autocorrelation"], rtol=1e-13, atol=1e-16)
    assert np.allclose(got["ic_correlation_blocks"].sum(axis=1), got["ic_correlation"], rtol=1e-13, atol=1e-16)


def test_rates_task_writes_the_error_and_the_next_batch_removes_it(tmp_path):
    from semiclassical_amd import driver as DR
    nt, B = 12, 4
    store, path = _store(tmp_path, nt)
    c, k = _batch(96, nt, 7)
    store.add_batch(c.sum(-1), k.sum(-1), 96, blocks=_blocks_of(c, k, B))
    task = {"task": "rates", "correlations": path, "rates": path, "broadening": "gaussian", "hwhmG_ev": 0.5}
    DR.calculate_rates(task)
    got = np.load(path)
    assert got["ic_rate_error"].shape == got["ic_rate"].shape and np.all(got["ic_rate_error"] > 0)
    lineshape, _ = DR.lineshape_from_task(task)
    e, sigma = rates.rate_standard_error(got["times"], got["ic_correlation_blocks"], got["block_trajectories"], lineshape)
    assert np.allclose(got["ic_rate_error"], (2.0 * np.pi * sigma)[e >= 0.0], rtol=1e-12, atol=0)
    store.add_batch(c.sum(-1), k.sum(-1), 96, blocks=_blocks_of(c, k, B))
    files = set(np.load(path).files)
    assert "ic_rate_error" not in files and "ic_rate" not in files and set(BLOCK_KEYS) <= files
    # a file without blocks gets a rate without an error
    plain, ppath = _store(tmp_path, nt, "plain.npz")
    plain.add_batch(c.sum(-1), k.sum(-1), 96)
    DR.calculate_rates(dict(task, correlations=ppath, rates=ppath))
    files = set(np.load(ppath).files)
    assert "ic_rate" in files and "ic_rate_error" not in files


def test_without_the_key_the_file_has_todays_keys(tmp_path):
    store, path = _store(tmp_path, 3)
    c, k = _batch(20, 3, 1)
    store.add_batch(c.sum(-1), k.sum(-1), 20)
    assert sorted(np.load(path).files) == sorted(TODAY)


def test_legacy_file_and_task_without_blocks_drop_the_block_keys(tmp_path, caplog):
    nt, B = 4, 8
    store, path = _store(tmp_path, nt)
    c, k = _batch(50, nt, 5)
    store.add_batch(c.sum(-1), k.sum(-1), 50)                                    # a legacy batch: no blocks
    keys = set(np.load(path).files)
    store.add_batch(c.sum(-1), k.sum(-1), 50, blocks=_blocks_of(c, k, B))        # blocks asked for, 50 stored trajectories have none
    assert set(np.load(path).files) == keys and "error blocks dropped" in caplog.text
    caplog.clear()
    store2, path2 = _store(tmp_path, nt, "second.npz")
    store2.add_batch(c.sum(-1), k.sum(-1), 50, blocks=_blocks_of(c, k, B))
    assert set(BLOCK_KEYS) <= set(np.load(path2).files)
    store2.add_batch(c.sum(-1), k.sum(-1), 50, blocks=_blocks_of(c, k, 4))       # another number of blocks cannot be pooled
    assert not set(BLOCK_KEYS) & set(np.load(path2).files) and "error blocks dropped" in caplog.text
    caplog.clear()
    store3, path3 = _store(tmp_path, nt, "third.npz")
    store3.add_batch(c.sum(-1), k.sum(-1), 50, blocks=_blocks_of(c, k, B))
    store3.add_batch(c.sum(-1), k.sum(-1), 50)                                   # the task no longer computes them
    assert not set(BLOCK_KEYS) & set(np.load(path3).files) and "error blocks dropped" in caplog.text


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_block_entry_points_are_declared_and_bound():
    from semiclassical_amd import _lib
    header = open(os.path.join(ROOT, "include", "semiclassical_hip.h")).read()
    for name in ("sc_term_blocks", "sc_term_blocks_at", "sc_hk_run_blocks"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.sc_abi_version() == 18 and _lib.ABI_VERSION == 18
    # the argument checks run before any launch: no GPU needed to be refused
    for bad in (0, 1, 3, 48, 128):
        assert _lib.lib.sc_term_blocks(8, None, 10, bad, 8, None) != 0
        assert _lib.lib.sc_hk_run_blocks(8, 10, 5, 1, bad, 8, None) != 0
    assert _lib.lib.sc_term_blocks(None, None, 10, 8, 8, None) != 0
    assert b"power of two" in _lib.lib.sc_last_error() or b"null" in _lib.lib.sc_last_error()
