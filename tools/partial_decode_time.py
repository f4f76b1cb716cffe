#!/usr/bin/env python3
"""Partial (spatially scalable) decode of one scalable-lifting slice (GPU box): the one-call host-tier
entry over the cloud a geometry decode leaves when it stops m octree levels early, next to the
whole-slice decode of the same cloud; per-kernel times from the context's profiler.
usage: partial_decode_time.py [points] [m]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g
g.load_package()
from mpeg_pcc_tmc13_amd import context, lift_params, lod_params, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
m_arg = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ctx = context(0)
xyz = synth.dense_cloud(n, seed=62, bits=11)[0]
N = len(xyz)
lp = lod_params()
lp.scalable_lifting_enabled_flag = 1
lp.max_neigh_range_minus1 = 4
rng = np.random.default_rng(62)
out = {}
for m in (0, m_arg):
    if m:
        order = np.argsort(synth.morton_codes(xyz), kind="stable")
        q = (xyz[order] >> m) << m
        _, first = np.unique(q, axis=0, return_index=True)
        cloud = np.ascontiguousarray(q[np.sort(first)] + (1 << (m - 1)), dtype=np.int32)
    else:
        cloud = xyz
    P = len(cloud)
    coeffs = (rng.integers(-40, 41, size=(P, 3)) * (rng.random((P, 3)) < 0.2)).astype(np.int32)

    def decode():
        lf = lift_params([P], qp=34)
        ctx.lift_decode_attr(lp, lf, cloud, coeffs, min_geom_node_size_log2=m, geom_num_points=N if m else None)
        return lf

    ms = []
    for rep in range(4):
        t = time.perf_counter()
        decode()
        ms.append((time.perf_counter() - t) * 1e3)
    ctx.set_profiling(True)
    lf = decode()
    kt = ctx.kernel_times()
    ctx.set_profiling(False)
    agg = {}
    for name, (t_ms, launches) in kt.items():
        key = name.rstrip("0123456789").rstrip("_")
        agg[key] = round(agg.get(key, 0.0) + t_ms, 3)
    out[f"m{m}"] = dict(slice_points=N, decoded_points=P, lods=int(lf.num_lods), host_call_ms=round(min(ms[1:]), 2),
                        kernels_ms_total=round(sum(agg.values()), 3),
                        kernels_ms=dict(sorted(agg.items(), key=lambda kv: -kv[1])[:10]))
print(json.dumps(out, indent=1))
