#!/usr/bin/env python
"""Record tests/golden/lu_tail_parent_bits.npz: the outputs of the register elimination for the dense states of
tests/tail_offpath_inputs.py (every shape of the last diagonal block), from the library of the commit BEFORE the determinant tail
left the item hand-over and the last block lost its dead work (GPU box only).

    (in a checkout of the parent commit)  python -m semiclassical_amd.build  and keep the library as var/libsc_parent.so
    SC_LIB_PATH=$PWD/var/libsc_parent.so python tools/record_lu_tail_parent_bits.py [out.npz]

The fixture holds outputs only (determinants, branch signs, flagged counts, a digest of the blocks) and the amplitude used per
dimension; the inputs are regenerated from the integer hash.  Per dimension the amplitude is the first of the ladder at which the
register elimination keeps at least half of the trajectories in every launch.  It must never be recorded with the library under
test: the script refuses to run without SC_LIB_PATH.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("SC_LIB_PATH"):
        sys.exit("set SC_LIB_PATH to the parent commit's library")
    from tests import tail_offpath_inputs as tin
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lu_tail_parent_bits.npz")
    data = {}
    for D in tin.DIMS:
        for amp in tin.LADDER:
            res = tin.run_paths(D, amplitude=amp)
            worst = max(int(res["pre_flagged"][0]), int(res["step_flagged"].max()))
            print(f"D={D} amplitude {amp}: flagged in the prefactor-only launch {int(res['pre_flagged'][0])} of {tin.NTRAJ}, "
                  f"in the steps {res['step_flagged'].tolist()}", flush=True)
            if 2 * worst <= tin.NTRAJ:
                break
        else:
            sys.exit(f"D={D}: no amplitude of the ladder keeps half of the trajectories in the register elimination")
        if amp != tin.AMPLITUDE[D]:
            print(f"D={D}: tests/tail_offpath_inputs.py AMPLITUDE has {tin.AMPLITUDE[D]}, the fixture is recorded at {amp}: update the table")
        data[f"amplitude_{D}"] = np.array([amp])
        for k, v in res.items():
            data[f"{k}_{D}"] = v
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
