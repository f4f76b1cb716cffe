"""The slices of the predicting encoder's finish (TEST INFRASTRUCTURE): noisy lidar-like reflectance with three
direct predictors at low QP -- the content whose whole-slice passes do not settle -- regenerated from seeds."""
import numpy as np

UNSETTLED_QPS = (10, 4)  # synth.lidar_cloud(40000, seed=21, refl_noise=24): 64 passes settle neither


def lidar(n=40000, seed=21, refl_noise=24):
    """-> xyz, reflectance [m,1] (8 bit), the LoD parameters of the predicting transform"""
    from mpeg_pcc_tmc13_amd import lod_params, synth
    xyz, attrs = synth.lidar_cloud(n, seed=seed, refl_noise=refl_noise)
    if attrs.max() > 255:
        attrs = attrs >> 8
    lp = lod_params(lifting=False, intra_range=64)
    lp.intra_lod_prediction_skip_layers = 0
    return xyz, np.ascontiguousarray(attrs[:, :1], dtype=np.int32), lp


def frame_of(xyz, attrs, seed=7):
    """a reference frame for the slice: the cloud jittered, a tenth of it dropped"""
    rng = np.random.default_rng(seed)
    keep = rng.random(len(xyz)) > 0.1
    xr = np.clip(xyz + rng.integers(-2, 3, size=xyz.shape), 0, None)[keep].astype(np.int32)
    ar = np.clip(attrs + rng.integers(-6, 7, size=attrs.shape), 0, 255)[keep].astype(np.int32)
    return xr, ar


def params(npl, lp, qp, direct=3):
    from mpeg_pcc_tmc13_amd import pred_params
    return pred_params(npl, qp=qp, chroma_offset=0, bitdepth=8, threshold=4, direct=direct, icp=False,
                       quant_neigh_weight=(0, 0, 0), max_levels=lp.num_detail_levels_minus1 + 1)
