#!/usr/bin/env python
"""Record tests/golden/rows5_parent_bits.npz: the five-sum rows of sc_hk_cross (diagonal and dense widths) and sc_hk_opcorr for
every shape and variant of tests/rows5_inputs.py, and the raw buffers of the two run() records there, from the commit BEFORE the
two families got one definition of their shared pieces (GPU box only).

    (in a checkout of the parent commit, with tests/rows5_inputs.py and this file copied in)
    python -m semiclassical_amd.build  and keep the library as var/libsc_parent.so
    SC_LIB_PATH=$PWD/var/libsc_parent.so python tools/record_rows5_parent_bits.py [out.npz]

The fixture holds outputs only; the inputs are regenerated from the integer hash.  It must never be recorded with the code under
test: the script refuses to run without SC_LIB_PATH, and where the propagators have the table of families.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("SC_LIB_PATH"):
        sys.exit("set SC_LIB_PATH to the parent commit's library")
    from semiclassical_amd import propagators
    from tests import rows5_inputs as rin
    if hasattr(propagators, "_ROW_FAMILIES"):
        sys.exit("these are the propagators under test: record in a checkout of the parent commit")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rows5_parent_bits.npz")
    data = {}
    for kernel in rin.KERNELS:
        for D in rin.DIMS:
            rows = rin.tile_rows(kernel, D)
            assert all(np.isfinite(v).all() for v in rows.values()), (kernel, D)
            print(f"{kernel} D={D}: {len(rows)} rows, largest entry {max(abs(v).max() for v in rows.values()):.3e}", flush=True)
            data.update(rows)
    for masked in (False, True):
        rows = rin.run_rows(masked)
        if masked:
            kept = rows["run_masked_kept"]
            print(f"masked run: kept {int(kept.sum())} of {kept.size}")
            assert 0 < kept.sum() < kept.size, "the median deviation has to discard some trajectories and keep some"
        assert all(np.isfinite(v).all() for v in rows.values()), masked
        data.update(rows)
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
