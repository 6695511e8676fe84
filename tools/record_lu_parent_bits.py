#!/usr/bin/env python
"""Record tests/golden/lu_parent_bits.npz: the outputs of the register elimination for the dense states of
tests/lu_trim_inputs.py, from the library of the commit BEFORE the elimination was trimmed (GPU box only).

    (in a checkout of the parent commit)  python -m semiclassical_amd.build  and keep the library as var/libsc_parent.so
    SC_LIB_PATH=$PWD/var/libsc_parent.so python tools/record_lu_parent_bits.py [out.npz]

The fixture holds outputs only (determinants, branch signs, flagged counts, a digest of the blocks); the inputs are regenerated
from the integer hash.  It must never be recorded with the library under test: the script refuses to run without SC_LIB_PATH.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("SC_LIB_PATH"):
        sys.exit("set SC_LIB_PATH to the parent commit's library")
    from tests import lu_trim_inputs as inp
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lu_parent_bits.npz")
    data = {}
    for D in inp.DIMS:
        res = inp.run_paths(D)
        for k, v in res.items():
            data[f"{k}_{D}"] = v
        print(f"D={D}: flagged in the prefactor-only launch {int(res['pre_flagged'][0])} of {inp.NTRAJ}, "
              f"in the steps {res['step_flagged'].tolist()}", flush=True)
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
