"""The register kernels for a constant dense Hessian at D <= 16 (csrc/sc_hk_step_lin.hip, csrc/sc_hk_run_lin.hip) after their shared
pieces got one definition (csrc/sc_lin16.h).  The bar is the bits of the commit before
(tests/golden/lin16_parent_bits.npz, recorded with the parent commit's library by tools/record_lin16_parent_bits.py from the same
integer-hash inputs, tests/lin16_inputs.py): no tolerance."""
import os

import numpy as np
import pytest

from tests import lin16_inputs as lin

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lin16_parent_bits.npz")


@pytest.fixture(scope="module")
def parent_bits():
    return dict(np.load(GOLDEN))


def _ids(cases):
    return [lin.tag(shape, n) for shape, n in cases]


def test_the_fixture_exercises_the_weak_pivot_routes(parent_bits):
    """identity + 0.4 noise: at least one trajectory of at least one shape was handed to the fix-up launch on the step path (the
    whole loop repeats the same eliminations in place); every case below reproduces these counts"""
    assert sum(int(v.sum()) for k, v in parent_bits.items() if k.endswith("_step_flagged")) > 0
    # ... and in the prefactor-only launch of the register kernel, for dense widths too (the general kernel flags nothing)
    assert sum(int(v.sum()) for k, v in parent_bits.items() if "_dense_" in k and k.endswith(("_pref0_flagged", "_pref1_flagged"))) > 0
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "rows5_parent_bits.npz"))


@pytest.mark.parametrize("shape,n", lin.cases(), ids=_ids(lin.cases()))
def test_every_route_of_the_parent(shape, n, parent_bits):
    """the prefactor-only launch of hk_step_lin_kernel (sc_hk_step, mode 1, with the dense descriptor: once without Phi, which stages
    zeros, once with it), three step() calls -- lin16_inputs asserts what the dispatcher asks for them, and with an all-zero state
    that the register kernel is what runs (every trajectory flagged) except for (5, 5, diagonal) (none) -- and, where
    hk_run_lin_kernel has the shape, which is asserted, run() of five steps with the product with Phi and (dense widths) in
    normal-mode coordinates, each with and without second moments: c2, sign, action, (q, p), flagged counts, energy log, raw slot and
    moment rows and the digest of the monodromy blocks of the parent commit, bit for bit (arrays of more than 1024 doubles as sha256).
    The engine's own prefactor at t = 0 (_prefactor_initial) is held too; it reaches neither kernel.  The host-built constants are
    compared first: a difference there is the host's linear algebra, not a kernel's."""
    host = f"{lin.tag(shape, 0)}_host_sha256"
    assert np.array_equal(lin.host_constants(shape), parent_bits[host]), \
        f"{host}: the HOST-built constants (Phi, L, R, overlap, normal modes) differ from the recording machine's -- not a kernel difference"
    got = lin.run_case(shape, n)
    expected = {k for k in parent_bits if k.startswith(lin.tag(shape, n) + "_")}
    assert set(got) == expected, sorted(set(got) ^ expected)
    different = [k for k, v in got.items() if not np.array_equal(v, parent_bits[k])]
    print(f"{len(got)} arrays, {len(different)} different from the parent's", different[:10])
    for k, v in got.items():
        assert v.shape == parent_bits[k].shape and np.array_equal(v, parent_bits[k]), k
