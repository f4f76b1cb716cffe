"""Child process of tests/test_gpu_pred_repair.py (TEST INFRASTRUCTURE): the library reads
GPCC_PRED_REPAIR_AFTER once per context, so every setting gets a process of its own.  Codes the two unsettled
slices through gpcc_pred_encode_attr and, over an inter structure, gpcc_pred_forward_inter, and writes values,
reconstructions and statistics to the .npz named on the command line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import conftest  # noqa: E402,F401  (the package under its importable name)
import pred_repair_cases as pc  # noqa: E402


def main(out):
    from mpeg_pcc_tmc13_amd import context
    ctx = context(0)
    xyz, attrs, lp = pc.lidar()
    res = {}
    for qp in pc.UNSETTLED_QPS:
        v, rec, _, idx = ctx.pred_encode_attr(lp, pc.params([len(xyz)], lp, qp), xyz, attrs)
        res[f"v{qp}"], res[f"rec{qp}"] = v, rec
    xr, ar = pc.frame_of(xyz, attrs)
    lod = ctx.lod_build_inter(lp, xyz, xr, 64, 1)
    v, rec = ctx.pred_inter(True, pc.params(lod["npl"], lp, 10), lod, ar, attrs=attrs)
    res["v_inter"], res["rec_inter"] = v, rec
    res["pass_stats"] = np.array(list(ctx.pred_pass_stats().values()), np.int64)
    res["repair_stats"] = np.array(list(ctx.pred_repair_stats().values()), np.int64)
    ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
