"""The pair kernel (sc_hk_step_multi) without its intermediate block store: sub-step 0 of a visit forms M1 = P(0) M0 in registers
only, the last sub-step loads M0 again, applies P(0) and then P(1) and stores M2.  A wrong P(0) or P(1) row, or the two in the
wrong order, is invisible on the benchmark's diagonal blocks (zeros stay zeros under any rotation), so everything here runs on the
DENSE states of tests/lu_trim_inputs.py.  The bar is bit-identity with two sc_hk_step launches: sep_propagate_row is explicit fma,
the recomputed M1 has the bits the one-step kernel stores and reloads.

The store-free scheme is compiled for NR >= 3 (D > 32, NOSTORE_MIN_NR in csrc/sc_hk_step_sd.hip): D = 33, 48, 60, 64 run the new
code; D = 17 and 20 (NR = 2) run the pair kernel that still stores after every sub-step and are here so that both sides of that
switch meet the same bar on dense blocks."""
import numpy as np
import pytest
import torch

from tests import lu_trim_inputs as inp

pytestmark = pytest.mark.gpu

# Amplitude of the off-diagonal noise of the dense states.  The comparison needs every INTERMEDIATE determinant to come from the
# register elimination on both sides: an unrepaired one (sc_multi_scratch.unrepaired != 0) is handed to the fully pivoted kernel by
# the one-step path only, and determinant and possibly the branch sign then differ legitimately.  The fixture's 0.3 does not give
# that, and neither does 0.05 (measured on MI355X: 4 ... 28 of 64 trajectories unrepaired at 0.3, 0 ... 18 at 0.05, growing with D):
# the prefactor matrix is not M but  1/2 [ sqrt(w_a/w_b) Mqq + sqrt(w_b/w_a) Mpp - i sqrt(w_a w_b) Mqp + i Mpq / sqrt(w_a w_b) ],
# and with w = 7e-4 ... 1.5e-2 a.u. the noise of Mpq enters 70 ... 1400 times enlarged.  Its largest ratio of off-diagonal row sum
# to diagonal element is 15600 * amplitude at D = 64 (less below; _row_dominance computes it).  1e-5 makes every matrix of every test
# here strictly row-diagonally dominant with a ratio below 1/4, which Gaussian elimination preserves: the diagonal element is the
# largest of its row at every stage, so no pivot is weak, for any D -- one amplitude for all.  The blocks stay dense (every element a
# full-mantissa double), which is all a bit-for-bit comparison needs to see a wrong or misplaced row propagator.
AMPLITUDE = 1e-5


def _row_dominance(D, y):
    """largest (sum of off-diagonal magnitudes) / (diagonal magnitude) over the rows of the prefactor matrices of the state y"""
    import bench
    n = y.shape[1]
    s = np.sqrt(bench.as60_model(D)[0].numpy())
    mqq, mqp, mpq, mpp = (y[2 * D + k * D * D: 2 * D + (k + 1) * D * D].reshape(D, D, n) for k in range(4))
    ab, ba, prod = (s[:, None] / s[None, :])[:, :, None], (s[None, :] / s[:, None])[:, :, None], (s[:, None] * s[None, :])[:, :, None]
    mag = np.abs(0.5 * (ab * mqq + ba * mpp - 1j * prod * mqp + 1j * mpq / prod))
    diag = np.einsum("aan->an", mag)
    return float(((mag.sum(axis=1) - diag) / diag).max())


def _pair_and_singles(D, y):
    """one sc_hk_step_multi launch and two sc_hk_step launches from the same state, both left in the tiled layout"""
    from semiclassical_amd import _lib
    a, pot = inp.engine(D, y)
    b, _ = inp.engine(D, y)
    desc = a._potential_descriptor(pot, inp.DT)
    a._launch_step_pair(desc, inp.DT)
    b.step(pot, inp.DT)
    b.step(pot, inp.DT)
    torch.cuda.synchronize()
    b._set_mono_layout(_lib.SC_MONO_TILED16)
    torch.cuda.synchronize()
    assert a._state.mono_layout == b._state.mono_layout == _lib.SC_MONO_TILED16
    return a, b


def _assert_same_bits(a, b):
    for name in ("_qp", "_act", "_mono", "_sgn"):
        x, z = getattr(a, name), getattr(b, name)
        print(name, "equal" if torch.equal(x, z) else f"DIFFERENT in {int((x != z).sum())} of {x.numel()} elements")
    print("_c2", "equal" if torch.equal(torch.view_as_real(a._c2), torch.view_as_real(b._c2)) else "DIFFERENT")
    for name in ("_qp", "_act", "_mono", "_sgn"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(torch.view_as_real(a._c2), torch.view_as_real(b._c2))


@pytest.mark.parametrize("D", [17, 20, 48, 60, 64])
def test_pairs_on_dense_blocks_every_tile_shape(D):
    """64 dense states per dimension: state, action, blocks, branch signs and determinants after one pair equal two single steps bit
    for bit, and no intermediate determinant was unrepaired.  Store-free path: D = 48 (NR = 3, full last tile), 60 (NR = 4, 12 rows /
    columns in the last tile), 64 (NR = 4, full); D = 17 and 20 (NR = 2, 1 and 4 rows in the last tile): the storing pair kernel"""
    _, y = inp.reference_state(D, inp.NTRAJ, amplitude=AMPLITUDE)
    dom = _row_dominance(D, y)
    a, b = _pair_and_singles(D, y)
    bad = int(a._multi["bad"].item())
    print(D, "amplitude", AMPLITUDE, "row dominance", dom, "unrepaired", bad)
    assert dom < 0.25
    assert bad == 0
    _assert_same_bits(a, b)


@pytest.mark.parametrize("D", [17, 33, 48])
def test_many_visits_per_workgroup_on_dense_blocks(D):
    """n = 3 * grid + 5: every persistent workgroup visits at least three trajectories -- both parities of the per-trajectory buffers,
    the re-read of the visit's blocks requested under sub-step 0's last diagonal block, and the next trajectory's first requests
    issued while the last sub-step's stores are outstanding.  D = 33 and 48 run the store-free path (NR = 3 with one row in the last
    tile and with a full one), D = 17 the storing pair kernel (NR = 2)"""
    from semiclassical_amd._lib import lib
    grid = lib.sc_step_grid(10 ** 6, D)
    n = 3 * grid + 5
    _, y = inp.reference_state(D, n, stream=5, amplitude=AMPLITUDE)
    dom = _row_dominance(D, y)
    a, b = _pair_and_singles(D, y)
    assert a._gstep == grid
    bad = int(a._multi["bad"].item())
    print(D, "n", n, "amplitude", AMPLITUDE, "row dominance", dom, "unrepaired", bad)
    assert dom < 0.25
    assert bad == 0
    _assert_same_bits(a, b)


@pytest.mark.parametrize("D", [60, 17])
def test_weak_pivot_in_the_last_sub_step_finds_its_blocks(D):
    """cyclically shifted blocks (every leading pivot of the register elimination is zero), as in
    tests/test_hk_multi_gpu.py::test_weak_pivot_in_an_intermediate_determinant_is_counted_and_raised: the fix-up launch of the last
    sub-step reads M2 from memory, where the last sub-step must have put it although nothing was stored in between.  Blocks,
    determinants and signs equal the one-step path; every trajectory is counted as unrepaired in the intermediate sub-step.
    D = 60 runs the store-free path, D = 17 the storing pair kernel (NR = 2)."""
    n = 50
    _, y = inp.reference_state(D, n)
    gen = torch.Generator().manual_seed(3)
    shift = torch.roll(torch.eye(D), 11, dims=1).unsqueeze(2).expand(-1, -1, n).clone() * (1.0 + 0.1 * torch.rand(D, D, n, generator=gen))
    zero = torch.zeros(D, D, n)
    for k, blk in enumerate([shift, zero, zero, shift.clone()]):
        y[2 * D + k * D * D: 2 * D + (k + 1) * D * D] = blk.reshape(D * D, n).numpy()
    a, b = _pair_and_singles(D, y)
    bad = int(a._multi["bad"].item())
    print(D, "unrepaired", bad, "of", n)
    _assert_same_bits(a, b)
    assert bad == n
