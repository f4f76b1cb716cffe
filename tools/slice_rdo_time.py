#!/usr/bin/env python3
"""The slice-level inter / intra decision of one reflectance lifting slice (GPU box): both candidates through the
one-call entry (gpcc_lift_encode_attr_rdo) next to the existing entries called one after the other
(gpcc_lod_build_inter + gpcc_lift_forward_inter for the inter candidate, gpcc_lift_encode_attr for the intra one);
host-call times and per-kernel times from the context's profiler.
usage: slice_rdo_time.py [points]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g
g.load_package()
from mpeg_pcc_tmc13_amd import context, lift_params, lod_params, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
ctx = context(0)
xyz, a = synth.lidar_cloud(n, seed=71, refl_noise=24)
attrs = np.ascontiguousarray(a[:, :1], dtype=np.int32)
rng = np.random.default_rng(72)
keep = rng.random(len(xyz)) > 0.1
xr = np.clip(xyz + rng.integers(-1, 2, size=xyz.shape), 0, None)[keep].astype(np.int32)
ar = np.clip(attrs + rng.integers(-5, 6, size=attrs.shape), 0, 255)[keep].astype(np.int32)
N = len(xyz)
lp = lod_params()
SEARCH = 128


def one_call():
    return ctx.lift_encode_attr_rdo(lp, lp, lift_params([N], qp=28, lcp=False), xyz, attrs, xr, ar, SEARCH, 1)


def two_entries():
    lod = ctx.lod_build_inter(lp, xyz, xr, SEARCH, 1)
    v0, r0 = ctx.lift_inter(True, lift_params(lod["npl"], qp=28, lcp=False), lod, ar, attrs=attrs)
    v1, r1, _, _ = ctx.lift_encode_attr(lp, lift_params([N], qp=28, lcp=False), xyz, attrs)
    # (the distortion sums, which the one call returns, on the host)
    return np.abs(r0.astype(np.int64) - attrs).sum(), np.abs(r1.astype(np.int64) - attrs).sum()


out = dict(points=N, frame_points=len(xr))
for label, fn in (("one_call", one_call), ("two_entries", two_entries)):
    ms = []
    for rep in range(4):
        t = time.perf_counter()
        res = fn()
        ms.append((time.perf_counter() - t) * 1e3)
    ctx.set_profiling(True)
    fn()
    kt = ctx.kernel_times()
    ctx.set_profiling(False)
    agg = {}
    for name, (t_ms, launches) in kt.items():
        key = name.rstrip("0123456789").rstrip("_")
        agg[key] = round(agg.get(key, 0.0) + t_ms, 3)
    out[label] = dict(host_call_ms=round(min(ms[1:]), 2), kernels_ms_total=round(sum(agg.values()), 3),
                      kernels_ms=dict(sorted(agg.items(), key=lambda kv: -kv[1])[:10]))
    if label == "one_call":
        out[label]["dist"] = [int(v) for v in res[2]]
        out[label]["slice_distortion_ms"] = agg.get("slice_distortion")
        if agg.get("slice_distortion"):
            # three arrays of N int32 read once
            out[label]["slice_distortion_GBps"] = round(12.0 * N / agg["slice_distortion"] / 1e6, 1)
    else:
        out[label]["dist"] = [int(v) for v in res]
print(json.dumps(out, indent=1))
