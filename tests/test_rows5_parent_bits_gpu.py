"""The five-sum rows of targets and operators (csrc/sc_rows5.h) after their shared pieces got one
definition: the accumulation of x, the column reduction, the reduction over the bands, and the launch orchestration of run().  The
bar is the bits of the commit before (tests/golden/rows5_parent_bits.npz, recorded with the parent commit's library and
propagators by tools/record_rows5_parent_bits.py from the same integer-hash inputs, tests/rows5_inputs.py)."""
import itertools
import os

import numpy as np
import pytest

from tests import rows5_inputs as rin

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows5_parent_bits.npz")


@pytest.fixture(scope="module")
def parent_bits():
    return dict(np.load(GOLDEN))


def _compare(got, parent_bits):
    different = [key for key, val in got.items() if not np.array_equal(val, parent_bits[key])]
    print(f"{len(got)} arrays, {len(different)} different from the parent's", different[:10])
    for key, val in got.items():
        assert val.shape == parent_bits[key].shape and np.array_equal(val, parent_bits[key]), key


@pytest.mark.parametrize("D", rin.DIMS)
@pytest.mark.parametrize("kernel", rin.KERNELS)
def test_tile_rows_of_the_parent(kernel, D, parent_bits):
    """n in 1, 63, 64, 65, 130 and count in 1, 3, 64, 65, 130, each without a mask, with the first 64 trajectories discarded and
    through a cursor of 2 into a NaN buffer of three rows: the (count, 5) rows of the parent commit, bit for bit.  (tile_rows asserts that the rows the
    cursor leaves alone stay NaN, the helpers of the GPU tests that the cursor is not advanced.)"""
    got = rin.tile_rows(kernel, D)
    assert len(got) == len(rin.SIZES_N) * len(rin.SIZES_COUNT) * len(rin.VARIANTS)
    for n, c, v in itertools.product(rin.SIZES_N, rin.SIZES_COUNT, rin.VARIANTS):
        assert got[f"{kernel}_D{D}_n{n}_c{c}_{v}"].shape == (c, 5)
    _compare(got, parent_bits)


@pytest.mark.parametrize("masked", [False, True], ids=["visits", "masked"])
def test_run_buffers_of_the_parent(masked, parent_bits):
    """hk_as33, five steps, moments, four blocks, two targets and three operator pairs.  One run() call with visits of three steps;
    and single steps in two calls of 2 and 3 with discard_nonsymplectic at the median deviation between them: raw slots[:, :4],
    moments, blocks, cross and opcorr rows of the parent commit, bit for bit"""
    got = rin.run_rows(masked)
    if masked:
        kept = got["run_masked_kept"]
        assert 0 < kept.sum() < kept.size
    _compare(got, parent_bits)
