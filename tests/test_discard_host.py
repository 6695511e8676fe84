"""Discarding trajectories that fail the symplecticity check, without a GPU: the driver key's configuration errors (raised before
any device is touched), CorrelationStore's pooling of the kept counts and its refusal to pool different estimators, and the
declared, exported and bound entry points with the argument checks that run before any launch."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TODAY = ["propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories"]
KEYS = ["symplecticity_steps", "symplecticity_max", "symplecticity_mean", "symplecticity_exceeding", "symplecticity_tolerance"]
DISCARD_KEYS = ["symplecticity_kept", "symplecticity_discard"]


class _TwoRanks(object):
    rank, world = 0, 2


def _task(tmp_path, **extra):
    # the model file does not exist: a task that got past the checks of its keys would fail on it, not on a device
    task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(tmp_path / "missing.dat")},
            "num_steps": 4, "time_step_fs": 0.1, "results": {"correlations": str(tmp_path / "c.npz")}}
    task.update(extra)
    return task


def test_the_driver_key_needs_period_tolerance_and_one_rank(tmp_path):
    from semiclassical_amd import driver as DR
    with pytest.raises(DR.ConfigurationError, match="check_symplecticity_every"):
        DR.run_semiclassical_dynamics(_task(tmp_path, discard_nonsymplectic=True, symplecticity_tolerance=1e-8), device="cuda")
    with pytest.raises(DR.ConfigurationError, match="check_symplecticity_every"):
        DR.run_semiclassical_dynamics(_task(tmp_path, discard_nonsymplectic=True, symplecticity_tolerance=1e-8,
                                            check_symplecticity_every=0), device="cuda")
    with pytest.raises(DR.ConfigurationError, match="symplecticity_tolerance"):
        DR.run_semiclassical_dynamics(_task(tmp_path, discard_nonsymplectic=True, check_symplecticity_every=2), device="cuda")
    with pytest.raises(DR.ConfigurationError, match="'discard_nonsymplectic' is not available with more than one rank"):
        DR.run_semiclassical_dynamics(_task(tmp_path, discard_nonsymplectic=True, check_symplecticity_every=2,
                                            symplecticity_tolerance=1e-8), device="cuda", comm=_TwoRanks())
    with pytest.raises(DR.ConfigurationError, match="discard_nonsymplectic"):
        DR.run_semiclassical_dynamics(_task(tmp_path, discard_nonsymplectic="yes", check_symplecticity_every=2,
                                            symplecticity_tolerance=1e-8), device="cuda")
    assert not os.path.exists(tmp_path / "c.npz")
    # complete keys get past the checks (and then miss the model file); false is today's task
    for extra in (dict(discard_nonsymplectic=True, check_symplecticity_every=2, symplecticity_tolerance=1e-8),
                  dict(discard_nonsymplectic=False)):
        with pytest.raises((OSError, IOError)):
            DR.run_semiclassical_dynamics(_task(tmp_path, **extra), device="cuda")


def _store(tmp_path, nt, name="correlations.npz"):
    from semiclassical_amd import driver as DR
    path = str(tmp_path / name)
    np.savez(path, propagator="HK", times=np.arange(nt, dtype=float), autocorrelation=np.zeros(nt, complex),
             ic_correlation=np.zeros(nt, complex), adiabatic_gap=np.nan, zero_point_energy=0.0, trajectories=0)
    return DR.CorrelationStore(path), path


def _corr(nt):
    c = np.full(nt, 0.5 + 0.1j)
    c[0] = 1.0
    return c, 0.1 * c


def _record(eps, steps, tol, discard):
    """what propagate_batch returns for per-trajectory deviations eps (checks, n); with `discard` the trajectories above the
    tolerance leave at their check: max and mean over those still kept before it, 'kept' after it"""
    if not discard:
        return {"steps": np.asarray(steps), "max": eps.max(axis=1), "mean": eps.mean(axis=1), "exceeding": (eps > tol).sum(axis=1),
                "tolerance": tol}
    alive, largest, mean, kept = np.ones(eps.shape[1], bool), [], [], []
    for e in eps:
        largest.append(e[alive].max())
        mean.append(e[alive].mean())
        alive &= e <= tol
        kept.append(alive.sum())
    return {"steps": np.asarray(steps), "max": np.array(largest), "mean": np.array(mean), "exceeding": (eps > tol).sum(axis=1),
            "tolerance": tol, "kept": np.array(kept), "discard": True}


def test_store_adds_the_kept_counts(tmp_path):
    from semiclassical_amd import driver as DR
    rng = np.random.default_rng(5)
    nt, steps, tol, sizes = 9, [0, 4, 8], 3.0e-8, (200, 57, 131)
    store, path = _store(tmp_path, nt)
    records = [_record(np.abs(rng.normal(0, 3e-8, (3, m))), steps, tol, True) for m in sizes]
    c, k = _corr(nt)
    for m, rec in zip(sizes[:2], records[:2]):                     # two batches of one run ...
        store.add_batch(c, k, m, symplecticity=rec)
    DR.CorrelationStore(path).add_batch(c, k, sizes[2], symplecticity=records[2])      # ... and a later run
    got = np.load(path)
    assert sorted(got.files) == sorted(TODAY + KEYS + DISCARD_KEYS)
    assert bool(got["symplecticity_discard"]) and int(got["trajectories"]) == sum(sizes)
    assert np.array_equal(got["symplecticity_kept"], sum(rec["kept"] for rec in records))
    assert np.all(np.diff(got["symplecticity_kept"]) <= 0) and 0 < got["symplecticity_kept"][-1] < sum(sizes)
    assert np.array_equal(got["symplecticity_exceeding"], sum(rec["exceeding"] for rec in records))
    assert np.array_equal(got["symplecticity_max"], np.max([rec["max"] for rec in records], axis=0))
    assert float(got["symplecticity_tolerance"]) == tol


def test_without_discarding_the_file_has_the_keys_it_had(tmp_path):
    store, path = _store(tmp_path, 4)
    c, k = _corr(4)
    eps = np.abs(np.random.default_rng(1).normal(0, 1e-8, (2, 30)))
    store.add_batch(c, k, 30, symplecticity=_record(eps, [0, 2], 1e-8, False))
    store.add_batch(c, k, 30, symplecticity=_record(eps, [0, 2], 1e-8, False))
    assert sorted(np.load(path).files) == sorted(TODAY + KEYS)


def test_different_estimators_are_not_pooled(tmp_path):
    from semiclassical_amd import driver as DR
    nt = 6
    c, k = _corr(nt)
    eps = np.abs(np.random.default_rng(2).normal(0, 1e-8, (2, 40)))
    discarding = _record(eps, [0, 3], 1e-8, True)
    cases = [("a file without checks, a discarding batch", None, discarding, "discard_nonsymplectic"),
             ("a file with checks only, a discarding batch", _record(eps, [0, 3], 1e-8, False), discarding, "discard_nonsymplectic"),
             ("a discarding file, a batch with checks only", discarding, _record(eps, [0, 3], 1e-8, False), "discard_nonsymplectic"),
             ("a discarding file, a batch without checks", discarding, None, "discard_nonsymplectic"),
             ("another tolerance", discarding, _record(eps, [0, 3], 2e-8, True), "tolerance"),
             ("other steps", discarding, _record(eps, [0, 4], 1e-8, True), "other steps")]
    for i, (what, first, second, text) in enumerate(cases):
        store, path = _store(tmp_path, nt, f"case{i}.npz")
        store.add_batch(c, k, 40, symplecticity=first)
        before = {key: value.copy() for key, value in np.load(path).items()}
        with pytest.raises(DR.ConfigurationError, match=text):
            store.add_batch(c, k, 40, symplecticity=second)
        after = dict(np.load(path))
        assert sorted(after) == sorted(before) and all(after[key].tobytes() == before[key].tobytes() for key in before), what
        store.add_batch(c, k, 40, symplecticity=first)            # the file is still good for batches of its own kind
        assert int(np.load(path)["trajectories"]) == 80


def test_entry_points_are_declared_exported_and_bound():
    from semiclassical_amd import _lib
    header = open(os.path.join(ROOT, "include", "semiclassical_hip.h")).read()
    assert re.search(r"\bint sc_discard_mark\(const double \*dev, int64_t n, double tol, int32_t step, uint8_t \*kept", header)
    assert re.search(r"\bint sc_term_masked_sums\(const double \*cq, const double \*kq, const uint8_t \*kept, int64_t n, int32_t B", header)
    assert re.search(r"\bint64_t sc_term_masked_scratch_doubles\(void\)", header)
    for name in ("sc_discard_mark", "sc_term_masked_sums", "sc_term_masked_scratch_doubles"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.sc_abi_version() == _lib.ABI_VERSION == 18
    assert _lib.lib.sc_term_masked_scratch_doubles() == 64 * 10
    # the argument checks run before any launch: no GPU needed to be refused
    lib = _lib.lib
    assert lib.sc_discard_mark(None, 4, 1e-3, 0, 16, 16, 16, None) == -1
    assert lib.sc_discard_mark(16, 4, 1e-3, 0, None, 16, 16, None) == -1
    assert lib.sc_discard_mark(16, 4, 1e-3, 0, 16, None, 16, None) == -1
    assert lib.sc_discard_mark(16, 4, 1e-3, 0, 16, 16, None, None) == -1
    for tol in (0.0, -1e-3, float("nan")):
        assert lib.sc_discard_mark(16, 4, tol, 0, 16, 16, 16, None) == -1
    assert lib.sc_term_masked_sums(None, None, 16, 4, 0, 16, 16, None, None, None) == -1
    assert lib.sc_term_masked_sums(16, None, None, 4, 0, 16, 16, None, None, None) == -1
    assert lib.sc_term_masked_sums(16, None, 16, 4, 0, None, 16, None, None, None) == -1
    assert lib.sc_term_masked_sums(16, None, 16, 4, 0, 16, None, None, None, None) == -1
    for B in (1, 3, 6, 128, -2):
        assert lib.sc_term_masked_sums(16, None, 16, 4, B, 16, 16, None, 16, None) == -1, B
    assert lib.sc_term_masked_sums(16, None, 16, 4, 8, 16, 16, None, None, None) == -1          # blocks wanted, no buffer
    assert lib.sc_term_masked_sums(16, None, 16, 4, 0, 16, 16, None, 16, None) == -1            # a buffer, no blocks
    assert lib.sc_term_masked_sums(8, None, 16, 4, 0, 16, 16, None, None, None) == -1           # cq not 16-byte aligned
    assert lib.sc_term_masked_sums(16, None, 18, 4, 0, 16, 16, None, None, None) == -1          # kept not 4-byte aligned
    from semiclassical_amd import propagators as PR
    for name in ("discard_nonsymplectic", "kept_count"):
        assert callable(getattr(PR.HermanKlukPropagator, name))
        assert getattr(PR.WaltonManolopoulosPropagator, name) is getattr(PR.HermanKlukPropagator, name)
    assert isinstance(PR.HermanKlukPropagator.kept, property) and isinstance(PR.HermanKlukPropagator.discarded_at, property)
