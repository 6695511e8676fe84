"""The per-step output rows of run() on the host: addresses and refusals of propagators._StepRows from CPU tensors, and
phased_cross against finalize_cross and against the algebra the driver used to carry itself.  No GPU."""
import numpy as np
import pytest
import torch

from semiclassical_amd import hostmath, units
from semiclassical_amd.propagators import HermanKlukPropagator, _StepRows

CPU = torch.device("cpu")
NT, B, K = 3, 4, 2


def _buffers(rows=5, dtype=torch.float64):
    return {"slots": torch.zeros((rows, 5), dtype=dtype), "moments": torch.zeros((rows, 6), dtype=dtype),
            "blocks": torch.zeros((rows, B, 4), dtype=dtype), "cross": torch.zeros((rows, K, 5), dtype=dtype)}


def test_row_addresses():
    """row k lies 40 k, 48 k, 32 B k and 40 K k bytes behind the bases, in buffers longer than nt as well; row k0 is where a
    whole-loop launch that starts at step k0 writes; absent buffers give None"""
    b = _buffers()
    rows = _StepRows(CPU, NT, **b, K=K)
    for k in range(5):
        row = rows.row(k)
        assert row.slot == b["slots"].data_ptr() + 40 * k
        assert row.moments == b["moments"].data_ptr() + 48 * k
        assert row.blocks == (b["blocks"].data_ptr() + 128 * k, B)
        assert row.cross == b["cross"].data_ptr() + 80 * k
        assert row.slots[row.k].data_ptr() == row.slot and row.slots[row.k].shape == (5,)
    piece = rows.row(2)
    assert (piece.slot, piece.moments, piece.blocks[0], piece.cross) == tuple(b[name][2:].data_ptr() for name in b)
    bare = _StepRows(CPU, NT, b["slots"]).row(1)
    assert bare.slot == b["slots"].data_ptr() + 40 and bare.moments is None and bare.blocks is None and bare.cross is None


def test_single_row():
    """the one-row constructor takes scratch of any shape and validates nothing: (8,), (5,) and (1, 5) slots, (1, K, 5) cross"""
    for slot in (torch.zeros(8, dtype=torch.float64), torch.zeros(5, dtype=torch.float64), torch.zeros((1, 5), dtype=torch.float64)):
        mom = torch.zeros((1, 6), dtype=torch.float64)
        row = _StepRows.single(slot, mom)
        assert (row.slot, row.moments, row.blocks, row.cross) == (slot.data_ptr(), mom.data_ptr(), None, None)
        row.slots[row.k][2:4] = torch.tensor([1.5, 2.5], dtype=torch.float64)          # what _generic_kic does with it
        assert slot.reshape(-1)[:5].tolist() == [0.0, 0.0, 1.5, 2.5, 0.0]
    out = torch.zeros((1, K, 5), dtype=torch.float64)
    row = _StepRows.single(cross=out)
    assert row.cross == out.data_ptr() and row.slot is None and row.moments is None


def _message(name, shape_text, device, got):
    return (f"{name} has to be a contiguous float64 tensor of shape {shape_text} on {device}, got {got.dtype} {tuple(got.shape)} "
            f"on {got.device}")


REFUSED = [("slots", "(>= 3, 5)", 5), ("moments", "(>= 3, 6)", 6), ("blocks", "(>= 3, B, 4)", 4), ("cross", "(>= 3, 2, 5)", 5)]


@pytest.mark.parametrize("name,shape_text,width", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals(name, shape_text, width):
    """every buffer: float32, a wrong trailing width, fewer than nt rows, a non-contiguous view, another device -- ValueError
    with the text run() has always raised"""
    good = _buffers()
    wider = torch.zeros(good[name].shape[:-1] + (2 * width,), dtype=torch.float64)
    bad = [_buffers(dtype=torch.float32)[name],                                  # dtype
           wider[..., :width + 1].contiguous(),                                  # trailing width
           good[name][:NT - 1],                                                  # rows
           wider[..., ::2]]                                                      # the right shape, not contiguous
    assert bad[3].shape == good[name].shape and not bad[3].is_contiguous()
    for t in bad:
        with pytest.raises(ValueError) as err:
            _StepRows(CPU, NT, **dict(good, **{name: t}), K=K)
        assert str(err.value) == _message(name, shape_text, "cpu", t)
    elsewhere = {n: t.to("meta") for n, t in good.items()}                      # one buffer on another device than the rest
    with pytest.raises(ValueError) as err:
        _StepRows(torch.device("meta"), NT, **dict(elsewhere, **{name: good[name]}), K=K)
    assert str(err.value) == _message(name, shape_text, "meta", good[name])
    assert str(err.value) == {"slots": "slots has to be a contiguous float64 tensor of shape (>= 3, 5) on meta, got torch.float64 (5, 5) on cpu",
                              "moments": "moments has to be a contiguous float64 tensor of shape (>= 3, 6) on meta, got torch.float64 (5, 6) on cpu",
                              "blocks": "blocks has to be a contiguous float64 tensor of shape (>= 3, B, 4) on meta, got torch.float64 (5, 4, 4) on cpu",
                              "cross": "cross has to be a contiguous float64 tensor of shape (>= 3, 2, 5) on meta, got torch.float64 (5, 2, 5) on cpu"}[name]


def test_refusals_of_counts():
    """B has to be a power of two in 2 ... 64; the K of cross has to be the targets'; something that is no tensor"""
    good = _buffers()
    for nblocks in (3, 128):
        with pytest.raises(ValueError) as err:
            _StepRows(CPU, NT, good["slots"], blocks=torch.zeros((NT, nblocks, 4), dtype=torch.float64))
        assert str(err.value) == f"the number of blocks has to be a power of two in 2 ... 64, got {nblocks}"
    with pytest.raises(ValueError) as err:
        _StepRows(CPU, NT, good["slots"], cross=good["cross"], K=K + 1)
    assert str(err.value) == _message("cross", "(>= 3, 3, 5)", "cpu", good["cross"])
    with pytest.raises(ValueError) as err:
        _StepRows(CPU, NT, [[0.0] * 5] * NT)
    assert str(err.value) == "slots has to be a contiguous float64 tensor of shape (>= 3, 5) on cpu, got <class 'list'> () on ?"


def test_no_steps():
    """nt = 0 with empty buffers is accepted, as run() has always accepted it (its loops then launch nothing).  The driver never
    asks for it: propagate_batch cuts [0, nt) at distinct steps, so every piece has at least one step, and with nt = 0 there is no
    piece at all."""
    b = {name: t[:0] for name, t in _buffers().items()}
    rows = _StepRows(CPU, 0, **b, K=K)
    assert (rows.B, rows.K) == (B, K)


def test_phased_cross():
    """finalize_cross is phased_cross + hostmath.standard_errors, bit for bit; phased_cross is the expression propagate_batch
    used to evaluate per piece"""
    rng = np.random.default_rng(5)
    raw = rng.normal(size=(4, 3, 5))
    raw[:, :, 2:4] = np.abs(raw[:, :, 2:4]) + 1.0
    t0, dt, E0, n = 7.25, 0.5, 0.013, 1000
    C, m3 = HermanKlukPropagator.phased_cross(torch.from_numpy(raw), t0, dt, E0)
    assert C.shape == (4, 3) and m3.shape == (4, 3, 3)
    C2, sigma = HermanKlukPropagator.finalize_cross(raw, t0, dt, E0, n)
    assert np.array_equal(C, C2) and np.array_equal(hostmath.standard_errors(C, m3, n), sigma)
    times_ = t0 + hostmath.time_grid(4, dt)
    X = (raw[:, :, 0] + 1j * raw[:, :, 1]) * np.exp(1j / units.hbar * times_ * E0)[:, None]
    m = hostmath.rotate_second_moments(raw[:, :, 2:5], (times_ * E0 / units.hbar)[:, None])
    assert np.array_equal(C, X) and np.array_equal(m3, m)
