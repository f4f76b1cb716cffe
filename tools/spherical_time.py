#!/usr/bin/env python3
"""Spherical-domain attribute positions of the 1 M-point lidar frame (GPU box): the device entry
(gpcc_dev_attr_to_spherical; HIP events on the context's stream, median of 20 behind a warm-up), its kernels one by
one (the context's profiler, median of 20), the host entry (wall time, PCIe both ways) and ten frames in one batch.
Prints ONE JSON line (profiles/spherical_time.jsonl collects them).

Per kernel: time, algorithmic bytes (12 read + 12 written per point and pass; the bounding-box pass of convert = 0
only reads) and their share of the 8 TB/s nominal roofline, as DESIGN.md section 5 accounts the other kernels.

The comparison figure is the reference's own convertXyzToRpl + offsetAndScale on one CPU core, which
tests/golden/make_spherical_golden.py prints where the reference tree exists; it comes from ANOTHER host than the
device numbers and is passed in: --reference-ms MS --reference-host "cpu model".
usage: spherical_time.py [--points N] [--reference-ms MS --reference-host TEXT]"""
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
from mpeg_pcc_tmc13_amd import spherical_params, synth  # noqa: E402
from mpeg_pcc_tmc13_amd.raht import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=1_000_000)
ap.add_argument("--reference-ms", type=float, default=None)
ap.add_argument("--reference-host", default=None)
args = ap.parse_args()

PEAK_BPS = 8e12
REPS = 20
dev = torch.device("cuda:0")
stream = torch.cuda.Stream(device=dev)
ctx = Context(0, stream=stream.cuda_stream)
xyz, _ = synth.lidar_cloud(args.points, seed=1)
n = len(xyz)
origin, thetas = synth.lidar_lasers()
# normalisedAxesWeights over {r, 25735, lasers - 1} for the 18-bit grid (encoder.cpp:190-212)
r = max(abs(int(origin[0])), abs((1 << 18) - 1 - int(origin[0])))
width = max(r + 1, 25736, len(thetas))
scale = [(width << 8) // (r + 1), (width << 8) // 25736, (width << 8) // len(thetas)]
p = spherical_params(origin, thetas, scale)


def device_ms(d_in, d_out, offsets, reps=REPS):
    """whole device-tier calls between two events on the context's stream"""
    ms = []
    for rep in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        ctx.dev_attr_to_spherical(p, offsets, d_in.data_ptr(), d_out.data_ptr())
        b.record(stream)
        ctx.synchronize()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms[3:])


def kernels_ms(d_in, d_out, offsets, reps=REPS):
    per = {}
    ctx.set_profiling(True)
    for rep in range(reps):
        ctx.dev_attr_to_spherical(p, offsets, d_in.data_ptr(), d_out.data_ptr())
        for name, (t_ms, launches) in ctx.kernel_times().items():
            per.setdefault(name, []).append(t_ms)
    ctx.set_profiling(False)
    return {k: statistics.median(v) for k, v in per.items()}


def account(name, ms, points):
    nbytes = {"rpl_convert": 24, "rpl_scale": 24, "rpl_bbox": 12}.get(name, 0) * points
    out = dict(ms=round(ms, 4), bytes=nbytes)
    if nbytes:
        out["GBps"] = round(nbytes / ms / 1e6, 1)
        out["share_of_8TBps"] = round(nbytes / (ms * 1e-3) / PEAK_BPS, 4)
    return out


d_in = torch.from_numpy(xyz.reshape(-1)).to(dev)
d_out = torch.empty_like(d_in)
torch.cuda.synchronize()
one = np.array([0, n], np.int64)
out = dict(tool="spherical_time", points=n, lasers=len(thetas), scale=scale, device=torch.cuda.get_device_name(0))
out["device_entry_ms"] = round(device_ms(d_in, d_out, one), 4)
out["kernels"] = {k: account(k, v, n) for k, v in kernels_ms(d_in, d_out, one).items()}
want = d_out.cpu().numpy().reshape(-1, 3)

# the host entry: pageable memory in, pageable memory out
ms = []
for rep in range(6):
    t = time.perf_counter()
    pos, bbox = ctx.attr_to_spherical(p, xyz)
    ms.append((time.perf_counter() - t) * 1e3)
assert np.array_equal(pos, want)
out["host_entry_ms"] = round(statistics.median(ms[1:]), 3)
out["bbox"] = bbox.reshape(-1).tolist()

# ten frames in one batch
frames = 10
d_in10 = d_in.repeat(frames)
d_out10 = torch.empty_like(d_in10)
torch.cuda.synchronize()
off10 = np.arange(frames + 1, dtype=np.int64) * n
out["batch10_device_entry_ms"] = round(device_ms(d_in10, d_out10, off10, reps=10), 4)
out["batch10_kernels"] = {k: account(k, v, frames * n) for k, v in kernels_ms(d_in10, d_out10, off10, reps=10).items()}
assert np.array_equal(d_out10.cpu().numpy().reshape(frames, -1, 3)[frames - 1], want)

if args.reference_ms is not None:
    out["reference_cpu"] = dict(ms=args.reference_ms, host=args.reference_host, what="convertXyzToRpl + offsetAndScale, -O3, one core, "
                                "best of five (tests/golden/make_spherical_golden.py); measured on another host than the device figures")
print(json.dumps(out))
