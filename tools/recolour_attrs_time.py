"""Two attributes of a slice: (a) two gpcc_recolour calls against (b) one gpcc_recolour_attrs call.

    python tools/recolour_attrs_time.py [--reps 10] [--tree DIR] [--no-check]

S-dense 1 M with a half-resolution target (colour 8 bit + a seeded 10-bit reflectance) and S-lidar 1 M at scale
0.25 (reflectance 8 bit + a seeded 8-bit colour).  After a warm-up of both forms, (a) and (b) alternate in one
process, a host clock around the synchronous calls: median / min / max per form, the kernel times of one profiled
repetition of each, and equality of (b) with (a) and with the compiled reference (the oracle where it is absent).
--tree DIR: load the package from another checkout; one without the new entry (the parent commit) times (a) alone,
the baseline."""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--no-check", action="store_true")
args = ap.parse_args()
sys.path.insert(0, args.tree)
sys.path.insert(0, os.path.join(args.tree, "tests"))
import __graft_entry__ as g  # noqa: E402
g.load_package()
from mpeg_pcc_tmc13_amd import context, recolour_params, synth  # noqa: E402
import oracle_loader as ol  # noqa: E402

ctx = context(0)
has_attrs = hasattr(ctx, "recolour_attrs")
tag = "attrs" if has_attrs else "parent"


def with_depth(p, d):
    q = type(p).from_buffer_copy(p)
    q.bitdepth = d
    return q


def stats(ms):
    return "median %.2f min %.2f max %.2f ms" % (np.median(ms), min(ms), max(ms))


for kind, n, scale in (("dense", 1_000_000, 0.5), ("lidar", 1_000_000, 0.25)):
    xyz, a = (synth.dense_cloud if kind == "dense" else synth.lidar_cloud)(n, seed=1)
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(len(xyz), -1)
    rng = np.random.default_rng(77)
    b = (rng.integers(0, 1024, (len(xyz), 1)) if kind == "dense" else rng.integers(0, 256, (len(xyz), 3))).astype(np.int32)
    attrs = [(a, 8), (b, 10 if kind == "dense" else 8)]
    tgt = np.unique(np.rint(xyz.astype(np.float64) * scale).astype(np.int32), axis=0)
    p = recolour_params()

    def two_calls():
        return [ctx.recolour(with_depth(p, d), xyz, v, tgt, scale=scale) for v, d in attrs]

    def one_call():
        return ctx.recolour_attrs(p, xyz, attrs, tgt, scale=scale)

    forms = [("a: two recolour calls", two_calls)] + ([("b: one recolour_attrs call", one_call)] if has_attrs else [])
    results = {name: f() for name, f in forms}  # warm-up of every form
    times = {name: [] for name, _ in forms}
    for _ in range(args.reps):
        for name, f in forms:
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    head = "%s %s ns %d nt %d reps %d" % (tag, kind, len(xyz), len(tgt), args.reps)
    for name, _ in forms:
        print(head, "|", name, "|", stats(times[name]), flush=True)
    ctx.set_profiling(True)
    for name, f in forms:
        ctx.kernel_times()
        f()
        kt = ctx.kernel_times()
        print(head, "|", name, "| kernel ms", {k: round(v[0], 3) for k, v in kt.items() if k.startswith("rc_")},
              "launches", {k: v[1] for k, v in kt.items() if k.startswith("rc_")}, flush=True)
    ctx.set_profiling(False)
    if has_attrs:
        same = all(np.array_equal(x, y) for x, y in zip(results[forms[0][0]], results[forms[1][0]]))
        print(head, "| b == a:", same, flush=True)
    if has_attrs and not args.no_check:
        checker, who = (ol.ref(), "compiled reference") if ol.ref_available() else (ol.oracle(), "oracle")
        t0 = time.perf_counter()
        want = [checker.recolour(with_depth(p, d), xyz, v, tgt, scale=scale) for v, d in attrs]
        t1 = time.perf_counter()
        agree = [float(np.all(x == y, axis=1).mean()) for x, y in zip(results[forms[1][0]], want)]
        print(head, "| b ==", who, "(two calls, %.2f s):" % (t1 - t0), agree, flush=True)
