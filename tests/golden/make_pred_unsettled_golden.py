#!/usr/bin/env python3
"""Generate tests/golden/pred_unsettled_golden.npz from the COMPILED REFERENCE at operator level (oracle/_ref:
AttributeEncoder::encode + AttributeDecoder::decode of the predicting transform, the symbols read back from the payload
by the reference's own entropy decoder) for the cases of tests/test_oracle_pred_unsettled.py: SHA-256 of the symbol
stream and of the reconstruction, the count of non-zero symbols, and one small case in full.  Inputs are regenerated
from the seeds (their SHA-256 is stored).  Run in the build container:
    make -C oracle && python tests/golden/make_pred_unsettled_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401
import test_oracle_pred_unsettled as tu  # noqa: E402


def main():
    out = {}
    for name in tu.CASES:
        kind, xyz, attrs = tu.inputs(name)[:3]
        values, rec = tu.reference(name)
        out[name + "/in_sha"] = np.array(tu.sha(xyz, attrs))
        out[name + "/values_sha"] = np.array(tu.sha(values))
        out[name + "/rec_sha"] = np.array(tu.sha(rec))
        out[name + "/nonzero"] = np.array(np.count_nonzero(values))
        if name == tu.FULL:
            out[name + "/values"] = np.asarray(values, dtype=np.int32)
            out[name + "/rec"] = np.asarray(rec, dtype=np.int32)
        print(f"{name:22s} {kind:6s} n={len(xyz):6d} c={attrs.shape[1]} nonzero symbols={np.count_nonzero(values)}")
    path = os.path.join(HERE, "pred_unsettled_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
