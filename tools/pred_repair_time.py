#!/usr/bin/env python3
"""Time of the predicting encoder's finish (GPU box): gpcc_pred_encode_attr -- LoD build, passes and ordered walk,
host buffers in and out -- on noisy lidar-like reflectance slices that 64 whole-slice passes do not settle, against
what declining them cost: the reference's coder for the same slice on one host core.

    python tools/pred_repair_time.py [--points 1000000] [--reps 10] [--warmup 2] [--sweep 2,4,8,16,32] [--out FILE]

One JSON line per measurement.  The entry is synchronous (it returns host arrays), so its time is the wall clock
around the call: median of --reps after --warmup calls on a context that has its arena.  The reference figures:
`reference_roundtrip_s` AttributeEncoder::encode + AttributeDecoder::decode out of oracle/_ref (the harness has no
encode-only entry), and `cpu_encode_lower_bound_s` = the reference's AttributeLods::generate + the serial port of
encodeReflectancesPred (oracle/pred_oracle.c), i.e. the reference's encode WITHOUT its entropy coder: the device has
to beat the latter to be worth keeping the slice.  --sweep times the same slices and the bench's dense colour slice at
several GPCC_PRED_REPAIR_AFTER (a context reads it when it is created)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

g.load_package()
import numpy as np  # noqa: E402
import lod_helpers as lh  # noqa: E402
import oracle_loader as ol  # noqa: E402
import pred_repair_cases as pc  # noqa: E402
from mpeg_pcc_tmc13_amd import context, lod_params, pred_params, synth  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def delta(ctx, before):
    p, r = ctx.pred_pass_stats(), ctx.pred_repair_stats()
    return {"passes": p["passes"] - before[0]["passes"], "declined": p["declined_at_the_limit"],
            "walked": r["walked"] - before[1]["walked"], "stretches": r["stretches"] - before[1]["stretches"],
            "longest_stretch": r["longest_stretch"]}


def lidar_line(ctx, xyz, attrs, lp, qp, reps, warmup, after):
    n = len(xyz)
    call = lambda: ctx.pred_encode_attr(lp, pc.params([n], lp, qp), xyz, attrs)
    med, lo, hi = timed(call, reps, warmup)
    ctx.set_profiling(True)
    ctx.kernel_times()
    before = (ctx.pred_pass_stats(), ctx.pred_repair_stats())
    v, rec, _, _ = call()
    kt = {k: round(t[0], 3) for k, t in ctx.kernel_times().items() if k.startswith("pred")}
    ctx.set_profiling(False)
    st = delta(ctx, before)
    line = {"slice": f"lidar_cloud({n}, seed=21, refl_noise=24) reflectance, 3 direct predictors, qp {qp}",
            "repair_after": after, "entry": "gpcc_pred_encode_attr", "device_s": round(med, 4), "device_min_s": round(lo, 4),
            "device_max_s": round(hi, 4), "reps": reps, "pred_kernels_ms": kt, **st}
    if st["walked"] and "pred_repair" in kt:
        line["walk_us_per_predictor"] = round(kt["pred_repair"] * 1e3 / st["walked"], 3)
    return line, v, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--sweep-reps", type=int, default=3)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    xyz, attrs, lp = pc.lidar(args.points)
    n = len(xyz)
    default_after = None
    if not args.sweep:
        ctx = context(0)
        for qp in (4, 10):
            line, v, rec = lidar_line(ctx, xyz, attrs, lp, qp, args.reps, args.warmup, "default")
            if not args.no_reference:
                t0 = time.perf_counter()
                lod = lh.oracle_lod_generate(xyz, lp)
                t_lod_port = time.perf_counter() - t0
                pp = pc.params(lod["npl"], lp, qp)
                t0 = time.perf_counter()
                wv, wrec, _, _ = lh.oracle_pred(True, pp, lod, attrs=attrs)
                t_pred = time.perf_counter() - t0
                line["equals_oracle"] = bool(np.array_equal(v, wv) and np.array_equal(rec, wrec))
                line["cpu_port_pred_encode_s"] = round(t_pred, 4)
                t_lod = t_lod_port
                kind = "port"
                if ol.ref_available():
                    t0 = time.perf_counter()
                    lh.ref_lod_generate(xyz, lp)
                    t_lod = time.perf_counter() - t0
                    kind = "reference"
                    t0 = time.perf_counter()
                    payload, re_, rd_, _ = lh.ref_pred_roundtrip(lp, pc.params([n], lp, qp), 4, qp, 0, xyz, attrs)
                    line["reference_roundtrip_s"] = round(time.perf_counter() - t0, 4)
                    line["reference_reconstruction_equal"] = bool(np.array_equal(re_, rec))
                line["cpu_lod_generate_s"] = round(t_lod, 4)
                line["cpu_lod_generate_kind"] = kind
                line["cpu_encode_lower_bound_s"] = round(t_lod + t_pred, 4)
                line["ratio_cpu_lower_bound_over_device"] = round((t_lod + t_pred) / line["device_s"], 3)
            emit(line)
        ctx.close()
        return
    # ---- the switch point ----
    dx, da = synth.dense_cloud(args.points, seed=41, bits=10 if args.points >= 500_000 else 8)
    dlp = lod_params(levels=12, lifting=False, intra_range=1100000, blend=True)
    dlp.intra_lod_prediction_skip_layers = 0
    for after in [int(t) for t in args.sweep.split(",")]:
        os.environ["GPCC_PRED_REPAIR_AFTER"] = str(after)
        ctx = context(0)
        for qp in (4, 10):
            line, _, _ = lidar_line(ctx, xyz, attrs, lp, qp, args.sweep_reps, 1, after)
            emit(line)
        m = len(dx)
        call = lambda: ctx.pred_encode_attr(dlp, pred_params([m], qp=28, bitdepth=8, max_levels=12, quant_neigh_weight=(16, 8, 4)), dx, da)
        before = (ctx.pred_pass_stats(), ctx.pred_repair_stats())
        med, lo, hi = timed(call, args.sweep_reps, 1)
        st = delta(ctx, before)
        emit({"slice": f"dense_cloud({m}) colour, CTC tools, qp 28 (bench.py's predicting slice)", "repair_after": after,
              "entry": "gpcc_pred_encode_attr", "device_s": round(med, 4), "device_min_s": round(lo, 4), "device_max_s": round(hi, 4),
              "reps": args.sweep_reps, "passes_per_call": st["passes"] / (args.sweep_reps + 1),
              "walked_per_call": st["walked"] / (args.sweep_reps + 1)})
        ctx.close()


if __name__ == "__main__":
    main()
