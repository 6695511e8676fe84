#!/usr/bin/env python
"""Record tests/golden/optile_parent_bits.npz: the rows of sc_hk_opquad and sc_hk_opcorr_thermal, the ket factors g of the three
pre-pass kernels (as SHA-256 of their bytes) for every shape and variant of tests/optile_inputs.py, and the raw buffers of the two
run() records there, from the commit BEFORE the operator tile kernels got one definition of their shared pieces (GPU box only).

    (in a checkout of the parent commit, with tests/optile_inputs.py and this file copied in)
    python -m semiclassical_amd.build  and keep the library as var/libsc_parent.so
    SC_LIB_PATH=$PWD/var/libsc_parent.so python tools/record_optile_parent_bits.py [out.npz]

The fixture holds outputs only; the inputs are regenerated from the integer hash.  It must never be recorded with the code under
test: the script refuses to run without SC_LIB_PATH, and where semiclassical_amd/csrc/sc_optile.h exists.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("SC_LIB_PATH"):
        sys.exit("set SC_LIB_PATH to the parent commit's library")
    if os.path.exists(os.path.join(ROOT, "semiclassical_amd", "csrc", "sc_optile.h")):
        sys.exit("this is the tree under test (csrc/sc_optile.h exists): record in a checkout of the parent commit")
    from tests import optile_inputs as oin
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "optile_parent_bits.npz")
    data = {}
    for kernel in oin.KERNELS:
        for D in oin.DIMS:
            rows = oin.TILE_ROWS[kernel](D)
            assert {k: v.shape for k, v in rows.items()} == oin.tile_keys(kernel, D), (kernel, D)
            assert all(np.isfinite(v).all() for v in rows.values()), (kernel, D)
            print(f"{kernel} D={D}: {len(rows)} arrays", flush=True)
            data.update(rows)
    for kind in oin.RUNS:
        rows = oin.run_rows(kind)
        assert all(np.isfinite(v).all() for v in rows.values()), kind
        print(f"run {kind}: " + ", ".join(f"{k} {v.shape}" for k, v in rows.items()), flush=True)
        data.update(rows)
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
