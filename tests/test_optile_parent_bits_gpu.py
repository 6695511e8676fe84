"""The tile and pre-pass kernels of the three operator families (sc_opcorr.hip, sc_opquad.hip, sc_thermal_opcorr.hip) after their
band header, staged loop, finish and affine dot got one definition in csrc/sc_optile.h, and the host's one
preparation of an operator pair.  The bar is the bits of the commit before (tests/golden/optile_parent_bits.npz, recorded with the
parent commit's library and propagators by tools/record_optile_parent_bits.py from the same integer-hash inputs,
tests/optile_inputs.py).  The rows of opcorr_tile_kernel are those of tests/test_rows5_parent_bits_gpu.py."""
import os

import numpy as np
import pytest

from tests import optile_inputs as oin

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optile_parent_bits.npz")


@pytest.fixture(scope="module")
def parent_bits():
    return dict(np.load(GOLDEN))


def _compare(got, parent_bits):
    different = [key for key, val in got.items() if not np.array_equal(val, parent_bits[key])]
    print(f"{len(got)} arrays, {len(different)} different from the parent's", different[:10])
    for key, val in got.items():
        assert val.shape == parent_bits[key].shape and val.dtype == parent_bits[key].dtype and np.array_equal(val, parent_bits[key]), key


@pytest.mark.parametrize("D", oin.DIMS)
@pytest.mark.parametrize("kernel", oin.KERNELS)
def test_tile_rows_of_the_parent(kernel, D, parent_bits):
    """opquad: n in 1, 64, 65, 130, seven (M, R_A) from two operators per tile to the wide path, R_B in 0, 3, each without a mask,
    with the first 64 trajectories discarded and through a cursor of 2 into a NaN buffer of three rows.  thermal: the same n, M in
    1, 3, 64, 65, d'' at the chunk edges of the mode loop, t in 0, 0.9, without and with the mask.  opcorr_initial: g alone.  The
    (M, 5) rows and the SHA-256 of every g (n, M) of the parent commit, bit for bit."""
    got = oin.TILE_ROWS[kernel](D)
    assert {key: val.shape for key, val in got.items()} == oin.tile_keys(kernel, D)
    _compare(got, parent_bits)


@pytest.mark.parametrize("kind", oin.RUNS)
def test_run_buffers_of_the_parent(kind, parent_bits):
    """hk_as33, five steps, moments, four blocks, three operator pairs: a K on the bra only in visits of three steps, and a thermal
    ensemble drawn on the device in pairs of steps.  Raw slots[:, :4], moments, blocks and opcorr / thermal_opcorr rows of the
    parent commit, bit for bit"""
    got = oin.run_rows(kind)
    assert set(got) == {f"run_{kind}_{k}" for k in ("slots", "moments", "blocks", "opcorr" if kind == "quadratic" else "thermal_opcorr")}
    _compare(got, parent_bits)
