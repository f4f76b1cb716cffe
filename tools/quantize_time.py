#!/usr/bin/env python3
"""gpcc_quantize_positions on a 1 M-point 12-bit sphere shell at scales 1, 0.5 and 0.125 (GPU box): 20 calls behind
3 warm-ups, timed by events on the context's stream; the host-tier call (uploads and downloads included) and, in a
second run of 20 calls with the context's profiler on, its kernels alone; gpcc_src_partition of the returned map (one
slice, every index) the same way.  Each result is checked against the digests the compiled reference left in
tests/golden/quantize_golden.npz.

The reference's times are the ones tests/golden/make_quantize_golden.py recorded in the golden file: one CPU core of
ANOTHER host than the device's (the reference tree does not travel with the package).  Both machines are named in
the output.  usage: quantize_time.py [--out FILE]   (profiles/quantize_time.txt keeps the lines)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import __graft_entry__ as g  # noqa: E402
g.load_package()
import quantize_cases as qc  # noqa: E402
from mpeg_pcc_tmc13_amd import quantize_params  # noqa: E402
from mpeg_pcc_tmc13_amd.raht import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()

WARM, REPS = 3, 20
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)
ctx = Context(0, stream=stream.cuda_stream)
gold = qc.golden()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def event_ms(fn):
    ms = []
    for rep in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms[WARM:]), min(ms[WARM:])


def kernels_ms(fn):
    """-> (ms per call of all kernels, {name: ms per call})"""
    ctx.set_profiling(True)
    ctx.kernel_times()
    for _ in range(REPS):
        fn()
    kt = ctx.kernel_times()
    ctx.set_profiling(False)
    per = {k: v[0] / REPS for k, v in kt.items()}
    return sum(per.values()), per


def groups(per):
    sort = sum(v for k, v in per.items() if k.startswith("qz_sort") or k == "qz_rekey")
    rest = {k: v for k, v in per.items() if not (k.startswith("qz_sort") or k == "qz_rekey")}
    return "sort passes %.3f" % sort + "".join(", %s %.3f" % (k, v) for k, v in sorted(rest.items()))


n = int(gold["timed/points"])
cloud = qc.sphere_shell(n)
props = torch.cuda.get_device_properties(0)
say(f"device: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); reference: {gold['timed/machine']} -- two different hosts")
say(f"cloud: {n} points on a 12-bit sphere shell; median (min) of {REPS} calls behind {WARM} warm-ups, ms")
for s1000, ref_us, uniq in zip(gold["timed/scales_x1000"], gold["timed/reference_us"], gold["timed/unique"]):
    scale = s1000 / 1000.0
    p = quantize_params(1, scale, clamp_min=(0, 0, 0), clamp_max=(4095, 4095, 4095))
    dst, idx, nxt = ctx.quantize_positions(p, cloud)
    ok = (len(idx) == int(uniq) and qc.digest(dst) == str(gold[f"timed/{scale}/dst_sha"])
          and qc.digest(idx) == str(gold[f"timed/{scale}/idx_sha"])
          and qc.digest(nxt) == str(gold[f"timed/{scale}/next_sha"]))
    med, best = event_ms(lambda: ctx.quantize_positions(p, cloud))
    ksum, per = kernels_ms(lambda: ctx.quantize_positions(p, cloud))
    say(f"quantize_positions scale {scale}: {len(idx)} unique, equal to the reference: {ok}; host-tier call "
        f"{med:.2f} ({best:.2f}); kernels alone {ksum:.3f}; reference quantizePositionsUniq {ref_us / 1000:.1f}")
    say(f"  kernels: {groups(per)}")
    every = np.arange(len(idx), dtype=np.int32)
    ox, _, _ = ctx.src_partition(cloud, None, idx, nxt, every, capacity=n)
    order = qc.partition(idx, nxt, every) if scale == 0.125 else None
    med, best = event_ms(lambda: ctx.src_partition(cloud, None, idx, nxt, every, capacity=n))
    ksum, per = kernels_ms(lambda: ctx.src_partition(cloud, None, idx, nxt, every, capacity=n))
    same = "" if order is None else f", equal to the restated walk: {bool((ox == cloud[order]).all())}"
    say(f"src_partition scale {scale}: one slice, {len(every)} indices, positions only{same}; host-tier call "
        f"{med:.2f} ({best:.2f}); kernels alone {ksum:.3f}")
    say("  kernels: " + ", ".join("%s %.3f" % (k, v) for k, v in sorted(per.items())))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
