"""Symplecticity check without a GPU: CorrelationStore's pooling of the new keys over batches and runs, the drop-with-warning
rule, the refusal under more than one rank, the declared entry point, and the host evaluation the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

from tests import symplectic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TODAY = ["propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories"]
KEYS = ["symplecticity_steps", "symplecticity_max", "symplecticity_mean", "symplecticity_exceeding", "symplecticity_tolerance"]


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


def _record(eps, steps, tol=None):
    """what propagate_batch returns for per-trajectory deviations eps (checks, n)"""
    rec = {"steps": np.asarray(steps), "max": eps.max(axis=1), "mean": eps.mean(axis=1)}
    if tol is not None:
        rec.update(exceeding=(eps > tol).sum(axis=1), tolerance=tol)
    return rec


def test_store_pools_the_checks_over_batches_and_runs(tmp_path):
    from semiclassical_amd import driver as DR
    rng = np.random.default_rng(3)
    nt, steps, tol, sizes = 9, [0, 4, 8], 3.0e-8, (200, 57, 131)
    store, path = _store(tmp_path, nt)
    eps = [np.abs(rng.normal(0, 3e-8, (3, m))) for m in sizes]
    c, k = _corr(nt)
    for e in eps[:2]:                                              # two batches of one run ...
        store.add_batch(c, k, e.shape[1], symplecticity=_record(e, steps, tol))
    DR.CorrelationStore(path).add_batch(c, k, sizes[2], symplecticity=_record(eps[2], steps, tol))      # ... and a later run
    got = np.load(path)
    assert sorted(got.files) == sorted(TODAY + KEYS)
    pooled = np.concatenate(eps, axis=1)
    assert np.array_equal(got["symplecticity_steps"], steps) and float(got["symplecticity_tolerance"]) == tol
    assert np.array_equal(got["symplecticity_max"], pooled.max(axis=1))
    assert np.allclose(got["symplecticity_mean"], pooled.mean(axis=1), rtol=1e-13, atol=0)
    assert np.array_equal(got["symplecticity_exceeding"], (pooled > tol).sum(axis=1))
    assert int(got["trajectories"]) == sum(sizes)


def test_without_a_tolerance_no_count_is_stored(tmp_path):
    store, path = _store(tmp_path, 4)
    c, k = _corr(4)
    eps = np.abs(np.random.default_rng(1).normal(0, 1e-8, (2, 30)))
    store.add_batch(c, k, 30, symplecticity=_record(eps, [0, 2]))
    store.add_batch(c, k, 30, symplecticity=_record(2 * eps, [0, 2]))
    got = np.load(path)
    assert sorted(got.files) == sorted(TODAY + KEYS[:3])
    assert np.array_equal(got["symplecticity_max"], 2 * eps.max(axis=1))
    assert np.allclose(got["symplecticity_mean"], 1.5 * eps.mean(axis=1), rtol=1e-14, atol=0)


def test_without_the_key_the_file_has_todays_keys(tmp_path):
    store, path = _store(tmp_path, 3)
    c, k = _corr(3)
    store.add_batch(c, k, 20)
    assert sorted(np.load(path).files) == sorted(TODAY)


def test_files_and_batches_that_do_not_match_drop_the_keys(tmp_path, caplog):
    nt = 6
    c, k = _corr(nt)
    eps = np.abs(np.random.default_rng(2).normal(0, 1e-8, (2, 40)))
    with_tol, other_tol = _record(eps, [0, 3], 1e-8), _record(eps, [0, 3], 2e-8)
    no_tol, other_steps = _record(eps, [0, 3]), _record(eps, [0, 4], 1e-8)

    store, path = _store(tmp_path, nt, "legacy.npz")
    store.add_batch(c, k, 40)                                      # stored trajectories without checks
    store.add_batch(c, k, 40, symplecticity=with_tol)
    assert sorted(np.load(path).files) == sorted(TODAY) and "symplecticity checks dropped" in caplog.text
    for i, second in enumerate((None, other_tol, no_tol, other_steps)):
        caplog.clear()
        store, path = _store(tmp_path, nt, f"case{i}.npz")
        store.add_batch(c, k, 40, symplecticity=with_tol)
        assert set(KEYS) <= set(np.load(path).files) and "dropped" not in caplog.text
        store.add_batch(c, k, 40, symplecticity=second)
        assert sorted(np.load(path).files) == sorted(TODAY), i
        assert "symplecticity checks dropped" in caplog.text
    caplog.clear()
    store, path = _store(tmp_path, nt, "notol.npz")               # a tolerance where the stored checks have none
    store.add_batch(c, k, 40, symplecticity=no_tol)
    store.add_batch(c, k, 40, symplecticity=with_tol)
    assert sorted(np.load(path).files) == sorted(TODAY) and "symplecticity checks dropped" in caplog.text


class _TwoRanks(object):
    rank, world = 0, 2


def test_more_than_one_rank_is_refused(tmp_path):
    from semiclassical_amd import driver as DR
    task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(tmp_path / "missing.dat")},
            "num_steps": 4, "time_step_fs": 0.1, "results": {"correlations": str(tmp_path / "c.npz")},
            "check_symplecticity_every": 2}
    with pytest.raises(DR.ConfigurationError, match="more than one rank"):
        DR.run_semiclassical_dynamics(task, device="cuda", comm=_TwoRanks())
    assert not os.path.exists(tmp_path / "c.npz")
    for bad in ({"check_symplecticity_every": -1}, {"check_symplecticity_every": 2.5}, {"symplecticity_tolerance": 0.0},
                {"symplecticity_tolerance": "1e-8"}):
        with pytest.raises(DR.ConfigurationError, match="symplecticity"):
            DR.run_semiclassical_dynamics(dict(task, **bad), device="cuda")


def test_entry_point_is_declared_exported_and_bound():
    from semiclassical_amd import _lib
    header = open(os.path.join(ROOT, "include", "semiclassical_hip.h")).read()
    assert re.search(r"\bint sc_symplectic_deviation\(const sc_state \*st, const double \*scale", header)
    assert "sc_symplectic_deviation" in _lib.SIGNATURES and hasattr(_lib.lib, "sc_symplectic_deviation")
    assert _lib.lib.sc_abi_version() == _lib.ABI_VERSION
    # the argument checks run before any launch: no GPU needed to be refused, and n = 0 is a no-op
    st = _lib.sc_state(n=0, dim=5, mono_layout=_lib.SC_MONO_ROWMAJOR, mono=8)
    assert _lib.lib.sc_symplectic_deviation(None, None, 8, None) == -1
    assert _lib.lib.sc_symplectic_deviation(st, None, None, None) == -1
    assert _lib.lib.sc_symplectic_deviation(st, None, 8, None) == 0
    for dim, layout, rc in ((0, 0, -2), (511, 0, -2), (65, _lib.SC_MONO_TILED16, -2), (60, 7, -1), (510, 0, 0), (64, 1, 0)):
        st = _lib.sc_state(n=0, dim=dim, mono_layout=layout, mono=8)
        assert _lib.lib.sc_symplectic_deviation(st, None, 8, None) == rc, (dim, layout)
    from semiclassical_amd import propagators as PR
    assert callable(PR.HermanKlukPropagator.symplectic_deviation)
    assert PR.WaltonManolopoulosPropagator.symplectic_deviation is PR.HermanKlukPropagator.symplectic_deviation


def test_host_evaluation_and_bound():
    """the yardstick of the GPU tests: exact on a planted defect, zero on the identity, and the bound scales as the derivation says"""
    D = 7
    blocks = np.zeros((2, 4, D, D))
    blocks[:, 0] = blocks[:, 3] = np.eye(D)
    blocks[1, 1, 2, 5] = 1e-6                                       # Mqp: E3 = B^T - B
    s = np.sqrt(np.arange(2.0, 2.0 + D))
    dev, bound = R.deviation_and_bound(blocks, s)
    assert np.array_equal(dev[0], [0.0, 0.0, 0.0])
    assert dev[1, 0] == 0.0 and dev[1, 1] == 0.0 and dev[1, 2] == 1e-6 * s[2] * s[5]
    # identity: S2 = 1 + 1 on the diagonal, largest weight s_b / s_a = 1 there -> 2 gamma_{2D+5} * 2
    assert np.isclose(bound[0, 1], 4 * R.gamma(2 * D + 5), rtol=1e-15) and R.gamma(3) == 3 * R.U / (1 - 3 * R.U)
    y = R.y_from_blocks(blocks)
    assert y.shape == (2 * D + 4 * D * D + 1, 2) and np.array_equal(R.blocks_from_y(y, D), blocks)
