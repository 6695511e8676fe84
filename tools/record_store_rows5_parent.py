#!/usr/bin/env python
"""Record tests/golden/store_rows5_parent.npz: every array CorrelationStore holds after each of the four add_batch calls of
tests/rows5_inputs.py (store_batches), and the warnings logged on the way, from the driver of the commit BEFORE the two families
of five-sum rows got one pooling rule (no GPU needed).

    (in a checkout of the parent commit, with tests/rows5_inputs.py and this file copied in)
    python tools/record_store_rows5_parent.py [out.npz]

It must never be recorded with the driver under test: the script refuses to run where the driver has the table of families.
"""
import logging
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Warnings(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.texts = []

    def emit(self, record):
        self.texts.append(record.getMessage())


def main():
    from semiclassical_amd import driver
    from tests import rows5_inputs as rin
    if hasattr(driver, "ROW_FAMILIES"):
        sys.exit("this is the driver under test: record in a checkout of the parent commit")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "store_rows5_parent.npz")
    seen = Warnings()
    driver.logger.addHandler(seen)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "correlations.npz")
        _, held = rin.replay_store(path)
    # the path of the file is part of every warning: the fixture holds the texts with the path cut out
    texts = [t.replace(path, "PATH") for t in seen.texts]
    for t in texts:
        print("warning:", t)
    for key, val in held.items():
        print(key, val.dtype, val.shape)
    np.savez_compressed(out, warnings=np.array(texts), **held)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
