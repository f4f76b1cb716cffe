"""Two attributes of a batch through the device tier's lifting coder: the LoD build per attribute against one build
and the batch transform over the held structure.

    python tools/dev_lift_time.py [--reps 10] [--out FILE] [--shapes 1x1000000,10x100000,64x16000]

Dense colour (c = 3, qp 31, 8 bit, last-component prediction) plus a 10-bit reflectance (c = 1, qp 43) on the same
geometry, for 1 x 1 M, 10 x 100 k and 64 x 16 k points; every slice is the seeded cloud in a shuffled point order of
its own.
(a) the way without the entries: gpcc_dev_lift_encode_attr once per attribute (each call builds the structure);
(b) gpcc_dev_lod_build once, then gpcc_dev_lift_forward once per attribute.
After a warm-up of both forms, (a) and (b) alternate in one process, a host clock around the work (every call returns
when its batch is done): median / min / max per form, one JSON line per shape.  The copy of the source attributes
into the buffers the coders work in is charged to both.  The outputs of the two forms are compared (coefficients,
reconstruction, LCP coefficients).  Launches: for (b) the spans of one profiled repetition (one span per launch in
lift_batch.hpp); for (a) the transform's launches follow from the LoD sizes (launch_lift's sequence, per slice and
attribute) and the LoD build's are given as the profiler's spans, which cover several launches each -- the build is
the same code in both forms, run twice in (a)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
ap.add_argument("--shapes", default="1x1000000,10x100000,64x16000")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
g.load_package()
import torch  # noqa: E402
from mpeg_pcc_tmc13_amd import context, lod_params, synth  # noqa: E402
from mpeg_pcc_tmc13_amd.params import lift_params_of_lod  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured")
dev = torch.device("cuda:0")
ctx = context(0)
out = open(args.out, "w") if args.out else None
ATTRS = [("colour", 3, dict(qp=31, bitdepth=8, lcp=True)), ("reflectance", 1, dict(qp=43, chroma_offset=0, bitdepth=10, lcp=False))]


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def launch_lift_launches(npl, c, lcp):
    """the launches of launch_lift's forward sequence for one slice"""
    steps = sum(1 for k in range(1, len(npl)) if npl[k] > npl[k - 1])
    return 1 + steps + 3 * steps + (2 if c == 3 and lcp else 0) + 1 + 3 * steps + 1


for shape in args.shapes.split(","):
    slices, per = (int(v) for v in shape.split("x"))
    bits = 10 if per >= 500_000 else 8
    xyz, colour = synth.dense_cloud(per, seed=1, bits=bits)
    n_s = len(xyz)
    refl = ((colour[:, :1] * 3 + colour[:, 1:2]) % 1024).astype(np.int32)
    perms = [np.random.default_rng(100 + s).permutation(n_s) for s in range(slices)]
    offsets = np.arange(slices + 1, dtype=np.int64) * n_s
    n = int(offsets[-1])
    lp = lod_params()
    d_xyz = torch.from_numpy(np.concatenate([xyz[q] for q in perms]).astype(np.int32)).to(dev)
    src = {"colour": torch.from_numpy(np.concatenate([colour[q] for q in perms]).astype(np.int32)).to(dev),
           "reflectance": torch.from_numpy(np.concatenate([refl[q] for q in perms])).to(dev)}
    res = {f: {name: dict(attrs=torch.zeros((n, c), dtype=torch.int32, device=dev),
                          coeffs=torch.zeros((n, c), dtype=torch.int32, device=dev), lcp=None)
               for name, c, _ in ATTRS} for f in "ab"}
    d_count, d_indexes = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
    d_index, d_weight = (torch.zeros(3 * n, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    ctx.set_morton_bits(3 * bits)
    held = {}

    def route_a():
        for name, c, kw in ATTRS:
            r = res["a"][name]
            r["attrs"].copy_(src[name])
            torch.cuda.synchronize()
            params = [lift_params_of_lod([1], **kw) for _ in range(slices)]
            r["lcp"] = ctx.dev_lift_attr(True, lp, params, offsets, d_xyz.data_ptr(), r["attrs"].data_ptr(),
                                         r["coeffs"].data_ptr(), c)
            ctx.synchronize()

    def route_b():
        held["npl"] = ctx.dev_lod_build(lp, offsets, d_xyz.data_ptr(), d_count.data_ptr(), d_index.data_ptr(),
                                        d_weight.data_ptr(), d_indexes.data_ptr())
        for name, c, kw in ATTRS:
            r = res["b"][name]
            r["attrs"].copy_(src[name])
            torch.cuda.synchronize()
            params = [lift_params_of_lod(row, **kw) for row in held["npl"]]
            r["lcp"] = ctx.dev_lift(True, params, offsets, d_count.data_ptr(), d_index.data_ptr(), d_weight.data_ptr(),
                                    d_indexes.data_ptr(), r["attrs"].data_ptr(), r["coeffs"].data_ptr(), c)

    forms = [("a_encode_attr_per_attribute", route_a), ("b_one_build_then_forward", route_b)]
    for _ in range(2):
        for _, f in forms:
            f()
    same = all(bool(torch.equal(res["a"][name][k], res["b"][name][k])) for name, _, _ in ATTRS for k in ("attrs", "coeffs"))
    same = same and all(np.array_equal(res["a"][name]["lcp"], res["b"][name]["lcp"]) for name, _, _ in ATTRS)
    assert same, "the two forms differ"
    times = {name: [] for name, _ in forms}
    for _ in range(args.reps):
        for name, f in forms:
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    spans = {}
    ctx.set_profiling(True)
    for name, f in forms:
        ctx.kernel_times()
        f()
        spans[name] = ctx.kernel_times()
    ctx.set_profiling(False)
    ctx.set_morton_bits(0)
    kb = spans["b_one_build_then_forward"]
    ka = spans["a_encode_attr_per_attribute"]
    rec = dict(tool="dev_lift_time", slices=slices, points_per_slice=n_s, reps=args.reps, outputs_equal=same,
               max_num_lods=max(len(v) for v in held["npl"]),
               nonzero_coeffs=int(sum(torch.count_nonzero(res["b"][name]["coeffs"]) for name, _, _ in ATTRS)))
    for name, _ in forms:
        rec[name] = stats(times[name])
    rec["b_over_a_median"] = round(rec["b_one_build_then_forward"]["median_ms"] / rec["a_encode_attr_per_attribute"]["median_ms"], 4)
    rec["a_lift_launches"] = int(sum(launch_lift_launches(row, c, kw["lcp"]) for row in held["npl"] for _, c, kw in ATTRS))
    rec["b_lift_launches"] = int(sum(v[1] for k, v in kb.items() if k.startswith("lift_batch_")))
    rec["a_lod_build_spans"] = int(sum(v[1] for k, v in ka.items() if not k.startswith("lift_")))
    rec["b_lod_build_spans"] = int(sum(v[1] for k, v in kb.items() if not k.startswith("lift_")))
    rec["b_lift_kernels_ms"] = {k: round(v[0], 4) for k, v in kb.items() if k.startswith("lift_batch_")}
    rec["a_lift_spans_ms"] = {k: round(v[0], 4) for k, v in ka.items() if k.startswith("lift_")}
    rec["b_lod_build_ms"] = round(sum(v[0] for k, v in kb.items() if not k.startswith("lift_")), 3)
    rec["a_lod_build_ms"] = round(sum(v[0] for k, v in ka.items() if not k.startswith("lift_")), 3)
    emit(rec)
