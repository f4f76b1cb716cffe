#!/usr/bin/env python3
"""LoD slices with attribute inter prediction and the crop of their reference frame (GPU box), median of 10 behind a
warm-up.  Prints ONE JSON line (profiles/inter_attr_time.jsonl collects them).

  * the 1 M-point lidar slice against a frame of the same size, lifting and predicting: the one-call host entry
    (gpcc_*_encode_attr_inter) against the two-call path (gpcc_lod_build_inter + gpcc_*_forward_inter) in the same
    process, wall time; and the device-tier entry between events on the context's stream;
  * gpcc_dev_attr_ref_crop of a 1 M-point frame against 1 and against 10 current slices: the call between events
    (it waits once on the stream), its kernels from the context's profiler, and per kernel the algorithmic bytes
    (count: 12 B per frame point and slice; scatter: 12 + 4c read per frame point and slice -- an upper bound, tiles
    that keep nothing return early -- plus 12 + 4c written per point kept) with their share of the 8 TB/s nominal.

The comparison figure of the crop is the fixture harness on one CPU core -- the crop restated with the reference's
computeBoundingBox and Box3::contains, not the reference encoder's own loop --, which
tests/golden/make_ref_crop_golden.py prints where the reference tree exists; it comes from ANOTHER host than the
device numbers and is passed in: --reference-ms MS1,MS10 --reference-host "cpu model".
usage: inter_attr_time.py [--points N] [--reference-ms MS1,MS10 --reference-host TEXT]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import __graft_entry__ as g  # noqa: E402
g.load_package()
from mpeg_pcc_tmc13_amd import lift_params, lod_params, pred_params, synth  # noqa: E402
from mpeg_pcc_tmc13_amd.raht import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=1_000_000)
ap.add_argument("--reference-ms", default=None)
ap.add_argument("--reference-host", default=None)
args = ap.parse_args()

PEAK_BPS = 8e12
REPS = 10
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)
ctx = Context(0, stream=stream.cuda_stream)
xyz, refl = synth.lidar_cloud(args.points, seed=1)
n = len(xyz)
rng = np.random.default_rng(2)
# the previous frame: the same scene, every point moved by at most one voxel, as many points as the slice
xr = np.clip(xyz + rng.integers(-1, 2, xyz.shape), 0, (1 << 18) - 1).astype(np.int32)
ar = np.clip(refl + rng.integers(-6, 7, refl.shape), 0, 255).astype(np.int32)
SEARCH, DIST = 128, 1


def median_ms(fn, reps=REPS):
    ms = []
    for rep in range(reps + 1):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms[1:]), 3)


def event_ms(fn, reps=REPS):
    ms = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        ctx.synchronize()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms[1:]), 3)


def blocks(predicting, npl):
    if predicting:
        lp = lod_params(lifting=False, intra_range=64)
        lp.intra_lod_prediction_skip_layers = 0
        return lp, pred_params(npl, qp=16, chroma_offset=0, bitdepth=8, threshold=4, direct=0, icp=False,
                               max_levels=lp.num_detail_levels_minus1 + 1)
    return lod_params(), lift_params(npl, qp=34, chroma_offset=0, lcp=False, bitdepth=8)


out = dict(tool="inter_attr_time", points=n, frame_points=len(xr), device=torch.cuda.get_device_name(0), reps=REPS)
d_xyz = torch.from_numpy(xyz.reshape(-1)).to(dev)
d_xr = torch.from_numpy(xr.reshape(-1)).to(dev)
d_ar = torch.from_numpy(ar.reshape(-1)).to(dev)
for predicting in (False, True):
    name = "pred" if predicting else "lift"
    lp, p = blocks(predicting, [n])
    res = {}

    def one_call():
        res["one"] = ctx.attr_inter(predicting, True, lp, blocks(predicting, [n])[1], xyz, xr, ar, SEARCH, DIST, attrs=refl)

    def two_calls():
        lod = ctx.lod_build_inter(lp, xyz, xr, SEARCH, DIST)
        fn = ctx.pred_inter if predicting else ctx.lift_inter
        res["two"] = fn(True, blocks(predicting, lod["npl"])[1], lod, ar, attrs=refl)

    t1, t2 = median_ms(one_call), median_ms(two_calls)
    assert np.array_equal(res["one"][0], res["two"][0]) and np.array_equal(res["one"][1], res["two"][1])
    d_a = torch.from_numpy(refl.reshape(-1)).to(dev)
    d_v = torch.zeros(n, dtype=torch.int32, device=dev)
    src = d_a.clone()
    torch.cuda.synchronize()

    def device_tier():
        d_a.copy_(src)
        ctx.dev_attr_inter(predicting, True, lp, [blocks(predicting, [n])[1]], [0, n], d_xyz.data_ptr(), d_a.data_ptr(),
                           d_v.data_ptr(), [0, len(xr)], d_xr.data_ptr(), d_ar.data_ptr(), SEARCH, DIST)

    with torch.cuda.stream(stream):
        t3 = event_ms(device_tier)
    assert np.array_equal(d_v.cpu().numpy(), res["one"][0][:, 0])
    out[name] = dict(one_call_host_ms=t1, two_call_host_ms=t2, device_tier_ms=t3)

# ---- the crop: the frame against 1 and against 10 current slices (the slice: the other frame, cut by index) ----
c = 1
for slices in (1, 10):
    off = np.linspace(0, n, slices + 1).astype(np.int64)
    cap = slices * len(xr)
    d_ox = torch.empty(3 * cap, dtype=torch.int32, device=dev)
    d_oa = torch.empty(c * cap, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    got = {}

    def crop():
        got["ro"] = ctx.dev_attr_ref_crop(off, d_xyz.data_ptr(), len(xr), d_xr.data_ptr(), d_ar.data_ptr(), c, d_ox.data_ptr(),
                                          d_oa.data_ptr(), cap)

    call_ms = event_ms(crop)
    per = {}
    ctx.set_profiling(True)
    for rep in range(REPS):
        crop()
        ctx.synchronize()
        for k, (t_ms, launches) in ctx.kernel_times().items():
            per.setdefault(k, []).append(t_ms)
    ctx.set_profiling(False)
    kept = int(got["ro"][-1])
    nbytes = {"ref_crop_count": 12 * len(xr) * slices, "slice_bbox": 12 * n,
              "ref_crop_scatter": (12 + 4 * c) * len(xr) * slices + (12 + 4 * c) * kept}
    kern = {}
    for k, v in per.items():
        ms = statistics.median(v)
        kern[k] = dict(ms=round(ms, 4))
        if k in nbytes and ms > 0:
            kern[k].update(bytes=nbytes[k], GBps=round(nbytes[k] / ms / 1e6, 1),
                           share_of_8TBps=round(nbytes[k] / (ms * 1e-3) / PEAK_BPS, 4))
    out[f"crop_{slices}"] = dict(call_ms=call_ms, kept=kept, kernels=kern)

if args.reference_ms is not None:
    ms = [float(v) for v in args.reference_ms.split(",")]
    out["reference_cpu"] = dict(ms_1_slice=ms[0], ms_10_slices=ms[1], host=args.reference_host,
                                what="the crop restated with the reference's computeBoundingBox + contains, -O3, one core, "
                                     "best of five (tests/golden/make_ref_crop_golden.py); measured on another host than "
                                     "the device figures")
print(json.dumps(out))
