"""Inputs and runs shared by tests/test_tail_offpath_gpu.py and tools/record_lu_tail_parent_bits.py (the recorder of
tests/golden/lu_tail_parent_bits.npz): the dense integer-hash states of tests/lu_trim_inputs.py at every shape of the LAST diagonal
block of the register elimination (csrc/sc_hk_lu.h)."""
from tests import lu_trim_inputs as inp

# rows of the last diagonal block / what the waves own there (wave w holds the rows 4 w .. 4 w + 3 of a 16-row slot):
#   17: one row (NR = 2), three waves leave at once     20: four rows, all in wave 0
#   33, 49: one row at NR = 3 and 4                     52: four rows at NR = 4
#   60: twelve rows, wave 3 has none                    61: thirteen rows, wave 3 has one      64: a full last block
DIMS = (17, 20, 33, 49, 52, 60, 61, 64)
NTRAJ = inp.NTRAJ
# Off-diagonal amplitude of the dense blocks per dimension: that of tests/lu_trim_inputs.py (0.3) wherever the register elimination
# of the PARENT commit's library keeps at least half of the 64 trajectories in every launch (counted when the fixture was recorded:
# the recorder lowers the amplitude of a dimension until that holds and writes it to the fixture, and the test compares it with this table)
AMPLITUDE = {D: inp.NOISE for D in DIMS}
LADDER = (0.3, 0.2, 0.1, 0.05, 0.02)


def run_paths(D, amplitude=None, n=NTRAJ):
    """tests.lu_trim_inputs.run_paths at the amplitude of this dimension: the prefactor-only launch and three sc_hk_step calls"""
    import hashlib
    import numpy as np
    import torch
    _, y = inp.reference_state(D, n, amplitude=AMPLITUDE[D] if amplitude is None else amplitude)
    prop, pot = inp.engine(D, y)
    out = {"pre_c2": prop._c2.cpu().numpy().copy(), "pre_sgn": prop._sgn.cpu().numpy().copy(),
           "pre_flagged": np.array([inp.flagged(prop)])}
    fl = []
    for _ in range(inp.NSTEPS):
        prop.step(pot, inp.DT)
        torch.cuda.synchronize()
        fl.append(inp.flagged(prop))
    out["step_c2"] = prop._c2.cpu().numpy().copy()
    out["step_sgn"] = prop._sgn.cpu().numpy().copy()
    out["step_flagged"] = np.array(fl)
    blocks = prop.y[2 * D:2 * D + 4 * D * D].cpu().numpy()
    out["blocks_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(blocks).tobytes()).digest(), dtype=np.uint8).copy()
    return out
