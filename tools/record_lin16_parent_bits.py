#!/usr/bin/env python
"""Record tests/golden/lin16_parent_bits.npz: every route of tests/lin16_inputs.py through hk_step_lin_kernel and hk_run_lin_kernel
(prefactor-only launch with the dense descriptor before and after Phi is attached, step(), run() with the product with Phi and in
normal-mode coordinates, with and without second moments; also the engine's own prefactor at t = 0, which reaches neither kernel),
from the commit BEFORE the two kernels got one definition of their shared pieces (GPU box only).

    (in a checkout of the parent commit) python -m semiclassical_amd.build  and keep the library as var/libsc_parent.so
    SC_LIB_PATH=$PWD/var/libsc_parent.so python tools/record_lin16_parent_bits.py [out.npz]

The fixture holds outputs and digests only; the inputs are regenerated from the integer hash.  It must never be recorded with the
code under test: the script refuses to run without SC_LIB_PATH.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("SC_LIB_PATH"):
        sys.exit("set SC_LIB_PATH to the parent commit's library")
    from tests import lin16_inputs as lin
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lin16_parent_bits.npz")
    data, flagged, flagged_pref_dense = {}, 0, 0
    for shape in lin.STEP_SHAPES:
        data[f"{lin.tag(shape, 0)}_host_sha256"] = lin.host_constants(shape)
    for shape, n in lin.cases():
        rows = lin.run_case(shape, n)
        assert all(np.isfinite(v).all() for v in rows.values() if v.dtype != np.uint8), (shape, n)
        fl = rows[f"{lin.tag(shape, n)}_step_flagged"]
        flagged += int(fl.sum())
        pref = [int(rows[f"{lin.tag(shape, n)}_{key}_flagged"][0]) for key in ("pref0", "pref1")]
        flagged_pref_dense += 0 if shape[2] else sum(pref)
        print(f"{lin.tag(shape, n)}: {len(rows)} arrays, flagged in the prefactor-only launches {pref}, per step {fl.tolist()}, "
              f"in the dispatch probe {int(rows[f'{lin.tag(shape, n)}_probe_flagged'][0])}", flush=True)
        data.update(rows)
    assert flagged > 0, "no trajectory took the fix-up launch on the step path"
    assert flagged_pref_dense > 0, "no trajectory of a dense-width shape was flagged in the prefactor-only launch"
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
