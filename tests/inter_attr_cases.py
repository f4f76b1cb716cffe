"""Slices with attribute inter prediction for the one-call and device-tier entries (TEST INFRASTRUCTURE): clouds and
reference frames from seeds, the parameter blocks of both transforms, and the CPU oracle chain of lod_helpers
(oracle_lod_generate_inter + lift_inter / pred_inter) they are compared with.

Every frame lies next to its slice (points of the slice moved by at most one voxel), so that the structure holds
neighbours in the frame: the tests assert that on the oracle's output."""
import numpy as np

import conftest  # noqa: F401  (makes the package importable)
import lod_helpers as lh
import oracle_loader as ol
from mpeg_pcc_tmc13_amd import lift_params, lod_params, pred_params, synth

BITDEPTH = 8
# the settings the device-tier shapes run with: frame_distance 1 and 2, search_range 0 and 128, lifting at QP 4 and
# 34, predicting with 0 and 3 direct predictors
SETTINGS = {
    "fd1_sr128": dict(frame_distance=1, search_range=128, qp=34, direct=3),
    "fd2_sr0": dict(frame_distance=2, search_range=0, qp=4, direct=0),
    # ... and the pairings the two above leave out: search_range 0 with frame_distance 1, QP 34 and direct predictors
    "fd1_sr0": dict(frame_distance=1, search_range=0, qp=34, direct=3),
    "fd2_sr128": dict(frame_distance=2, search_range=128, qp=4, direct=0),
}
GRID_N, GRID_NF = (1, 2, 65, 1025), (1, 64, 1500)


def slice_and_frame(n, nf, seed):
    """-> xyz [n,3], attrs [n,1], xyz_ref [nf,3], attrs_ref [nf,1]: a random cloud in a 32^3 cube and a frame of nf
    of its points (drawn with replacement) moved by at most one voxel, reflectances by at most 6"""
    xyz, attrs = synth.random_cloud(n, seed=seed, bits=5, c=1)
    rng = np.random.default_rng(seed + 100000)
    pick = rng.integers(0, n, nf)
    xr = np.clip(xyz[pick] + rng.integers(-1, 2, (nf, 3)), 0, 31).astype(np.int32)
    ar = np.clip(attrs[pick] + rng.integers(-6, 7, (nf, 1)), 0, 255).astype(np.int32)
    return np.ascontiguousarray(xyz, np.int32), np.ascontiguousarray(attrs, np.int32), xr, ar


def grid_batch(seed=900):
    """every n of GRID_N against every frame size of GRID_NF: twelve slices -> list of (xyz, attrs, xr, ar)"""
    return [slice_and_frame(n, nf, seed + 10 * i + j) for i, n in enumerate(GRID_N) for j, nf in enumerate(GRID_NF)]


def ragged_batch(seed=950, slices=40):
    """40 slices of 1..300 points with frames of 1..300 points"""
    rng = np.random.default_rng(seed)
    return [slice_and_frame(int(rng.integers(1, 301)), int(rng.integers(1, 301)), seed + 1 + s) for s in range(slices)]


def lod(predicting):
    if not predicting:
        return lod_params()
    lp = lod_params(lifting=False, intra_range=64)
    lp.intra_lod_prediction_skip_layers = 0
    return lp


def params(predicting, lp, npl, qp, direct):
    if not predicting:
        return lift_params(npl, qp=qp, chroma_offset=0, lcp=False, bitdepth=BITDEPTH)
    return pred_params(npl, qp=qp, chroma_offset=0, bitdepth=BITDEPTH, threshold=4, direct=direct, icp=False,
                       max_levels=lp.num_detail_levels_minus1 + 1)


def oracle(predicting, xyz, attrs, xr, ar, search_range, frame_distance, qp, direct):
    """the CPU oracle chain -> dict(values [n,1] coding order, recon [n,1] point order, indexes [n], npl,
    flagged: neighbours that live in the frame, frame_hits: the frame points they are)"""
    lp = lod(predicting)
    st = lh.oracle_lod_generate_inter(xyz, xr, lp, search_range, frame_distance)
    p = params(predicting, lp, st["npl"], qp, direct)
    if predicting:
        v, rec, _ = lh.pred_inter(True, p, st, ar, attrs=attrs)
    else:
        v, rec = lh.lift_inter(ol.oracle(), True, p, st, attrs, ar)
    used = np.arange(3)[None, :] < st["nc"][:, None]
    in_frame = st["ref"].astype(bool) & used
    return dict(values=v, recon=rec, indexes=st["indexes"], npl=st["npl"], flagged=int(in_frame.sum()),
                frame_hits=st["ni"][in_frame])
