"""CorrelationStore pools the five-sum rows of targets and of operators by one rule (driver.ROW_FAMILIES).  The bar is the file the
parent commit's two pooling blocks wrote: tests/golden/store_rows5_parent.npz, recorded by tools/record_store_rows5_parent.py
after each of the four add_batch calls of tests/rows5_inputs.py, with the warnings logged on the way."""
import logging
import os

import numpy as np
import pytest

from tests import rows5_inputs as rin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store_rows5_parent.npz")


def test_the_parent_file_after_every_batch(tmp_path, caplog):
    want = dict(np.load(GOLDEN))
    texts = [str(t) for t in want.pop("warnings")]
    path = str(tmp_path / "correlations.npz")
    with caplog.at_level(logging.WARNING, logger="semiclassical_amd.driver"):
        _, held = rin.replay_store(path)
    assert set(held) == set(want)
    for key, val in held.items():
        assert val.dtype == want[key].dtype and np.array_equal(val, want[key]), key
    for key in ("cross_correlation_error", "operator_correlation_error"):          # the sequence does reach the error keys
        assert "after1_" + key in held and "after2_" + key not in held
    got = [r.getMessage().replace(path, "PATH") for r in caplog.records if r.levelno == logging.WARNING]
    assert got == texts and len(texts) > 0


@pytest.mark.parametrize("family", ["cross", "operators"])
def test_refusals(family, tmp_path):
    """other targets or operators than the stored ones, and a family on one side only: ConfigurationError, from add_batch and
    from start() alike"""
    from semiclassical_amd import driver
    store, _ = rin.replay_store(str(tmp_path / "correlations.npz"))
    first = lambda: rin.store_batches()[0]
    add = lambda to, kw: to.add_batch(kw.pop("autocorrelation"), kw.pop("ic_correlation"), kw.pop("ntraj"), **kw)
    other = first()
    ident = "q" if family == "cross" else "ket_m"
    other[family] = dict(other[family], **{ident: other[family][ident] + 1.0})
    with pytest.raises(driver.ConfigurationError, match="other (targets|operators) than this task's"):
        add(store, other)
    absent = first()
    del absent[family]
    with pytest.raises(driver.ConfigurationError, match="cannot be pooled"):
        add(store, absent)
    # a file without the family, a batch with it
    bare = driver.CorrelationStore(str(tmp_path / "bare.npz"))
    bare.start({"results": {"overwrite": True}}, "HK", rin.store_times(), rin._Setup())
    kw = first()
    del kw[family]
    add(bare, kw)
    with pytest.raises(driver.ConfigurationError, match="holds no (cross-correlation|operator correlation) functions"):
        add(bare, first())
    # start() of a task that adds to the file
    q, p = first()["cross"]["q"], first()["cross"]["p"]
    ops = tuple(first()["operators"][key] for key in ("bra_c", "bra_m", "ket_c", "ket_m"))
    task = {"results": {"overwrite": False}}
    times = rin.store_times()
    store.start(task, "HK", times, rin._Setup(), cross_targets=(q, p), operators=ops)
    given = dict(cross_targets=(q, p), operators=ops)
    key = "cross_targets" if family == "cross" else "operators"
    with pytest.raises(driver.ConfigurationError, match="cannot be pooled"):
        store.start(task, "HK", times, rin._Setup(), **dict(given, **{key: None}))
    with pytest.raises(driver.ConfigurationError, match="other (targets|operators) than this task's"):
        store.start(task, "HK", times, rin._Setup(), **dict(given, **{key: tuple(a + 1.0 for a in given[key])}))
