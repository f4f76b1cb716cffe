#!/usr/bin/env python3
"""Generate tests/golden/ref_crop_golden.npz from the COMPILED REFERENCE: the previous frame cropped to the current
slice's bounding box, i.e. what encoder.cpp:1215-1236 / decoder.cpp:926-947 do in front of the lifting and
predicting coders of a slice with attribute inter prediction.

Per case of tests/ref_crop_cases.py and per slice, the harness next to this file (ref_crop_harness.cpp: the
reference's computeBoundingBox over the slice, its Box3::contains over every frame point) runs over the case's
clouds.  Stored per case: the slices' boxes, the offsets of the cropped frames back to back, SHA-256 digests of the kept positions
and attributes; for cases of at most FULL_MAX frame points the two arrays in full as well.  The input of the case
"lidar8" -- two frames of the synthetic lidar (consecutive seeds) moved into the spherical domain by the
reference's convertXyzToRpl + offsetAndScale (make_spherical_golden.py's harness) -- is stored too.

Both harnesses are compiled into a temporary directory; this runs only where the reference tree exists.  The
generator also prints the time of that restatement (the box and the walk with the reference's two functions, not the
reference encoder's own loop) for a 1 M-point frame on one core of the machine it runs on (tools/inter_attr_time.py
quotes it next to the device's)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)
import conftest  # noqa: E402,F401
import make_spherical_golden as msg  # noqa: E402
import ref_crop_cases as rc  # noqa: E402
import spherical_cases as sc  # noqa: E402
from mpeg_pcc_tmc13_amd import synth  # noqa: E402

REF = os.environ.get("GPCC_REFERENCE", "/root/reference")


def build_harness(tmp, opt="-O2"):
    so = os.path.join(tmp, "libref_crop_harness.so")
    cmd = ["g++", opt, "-DNDEBUG", "-std=c++11", "-fPIC", "-shared", "-w", "-I" + REF, "-I" + os.path.join(REF, "tmc3"),
           os.path.join(HERE, "ref_crop_harness.cpp"), "-o", so]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(so)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.ref_crop_ref.restype = C.c_int32
    lib.ref_crop_ref.argtypes = [i32p, C.c_int32, i32p, i32p, C.c_int32, C.c_int32, i32p, i32p, i32p,
                                 C.POINTER(C.c_int64)]
    return lib


def ref_crop(lib, xyz, frame_xyz, frame_attrs):
    """one slice -> (bbox [6], kept positions, kept attributes, nanoseconds)"""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    fx = np.ascontiguousarray(frame_xyz, dtype=np.int32)
    fa = np.ascontiguousarray(frame_attrs, dtype=np.int32)
    assert min(xyz.min(), fx.min()) >= 0 and max(xyz.max(), fx.max()) < (1 << 21)
    nf, c = fa.shape
    bbox = np.zeros(6, np.int32)
    ox, oa = np.zeros((nf, 3), np.int32), np.zeros((nf, c), np.int32)
    ns = C.c_int64(0)
    k = lib.ref_crop_ref(xyz.reshape(-1), len(xyz), fx.reshape(-1), fa.reshape(-1), nf, c, bbox, ox.reshape(-1),
                         oa.reshape(-1), C.byref(ns))
    return bbox, ox[:k].copy(), oa[:k].copy(), ns.value


def lidar_inputs(tmp):
    """frame t (whole, with its reflectances) and frame t + 1 in the spherical domain, as an inter-coded sequence
    has them: the minimum of the offset is zero (min_pos_mode 1) so that both frames share one domain"""
    lib = msg.build_harness(tmp)
    origin, thetas = synth.lidar_lasers()
    scale = msg.ref_scale(lib, sc.rmax("lidar_2000_s1"), len(thetas))
    out = []
    for seed in rc.LIDAR_SEEDS:
        xyz, refl = synth.lidar_cloud(rc.LIDAR_POINTS, seed=seed)
        _, _, pos, _, _ = msg.ref_slice(lib, origin, thetas, xyz, 1, 1, (0, 0, 0), scale)
        out.append((pos, refl))
    return {"lidar8/in_frame_xyz": out[0][0], "lidar8/in_frame_attrs": out[0][1].astype(np.int32),
            "lidar8/in_xyz": out[1][0]}


def main():
    assert os.path.isdir(os.path.join(REF, "tmc3")), "the reference tree is needed to regenerate this fixture"
    out = {"names": np.array(rc.NAMES)}
    with tempfile.TemporaryDirectory() as tmp:
        out.update(lidar_inputs(tmp))
        lib = build_harness(tmp)
        for name in rc.NAMES:
            c = rc.inputs(name, stored=out)
            off = c["offsets"]
            boxes, oxs, oas, ro = [], [], [], [0]
            for s in range(len(off) - 1):
                bbox, ox, oa, _ = ref_crop(lib, c["xyz"][off[s]:off[s + 1]], c["frame_xyz"], c["frame_attrs"])
                boxes.append(bbox)
                oxs.append(ox)
                oas.append(oa)
                ro.append(ro[-1] + len(ox))
            ox, oa = np.concatenate(oxs), np.concatenate(oas)
            res = {"bbox": np.stack(boxes), "ref_offsets": np.array(ro, np.int64), "xyz_sha": np.array(rc.digest(ox)),
                   "attrs_sha": np.array(rc.digest(oa))}
            if len(c["frame_xyz"]) <= rc.FULL_MAX:
                res["ref_xyz"], res["ref_attrs"] = ox, oa
            for k, v in res.items():
                out[f"{name}/{k}"] = v
            print(name, "frame", len(c["frame_xyz"]), "slices", len(off) - 1, "kept", ro[-1])
        # what the tests of those names rely on
        kept = np.diff(out["ragged300/ref_offsets"])
        sizes = np.diff(rc.inputs("ragged300")["offsets"])
        assert (kept == 0).sum() >= 10 and (kept > sizes).sum() >= 10, ((kept == 0).sum(), (kept > sizes).sum())
        kept = np.diff(out["lidar8/ref_offsets"])
        assert (kept > 0).all() and (kept < rc.LIDAR_POINTS).any(), kept
    with tempfile.TemporaryDirectory() as tmp:
        # the comparison figure of tools/inter_attr_time.py: a 1 M-point frame, -O3, one core, best of five
        lib = build_harness(tmp, "-O3")
        fx, fa = synth.lidar_cloud(1000000, seed=1)
        cur, _ = synth.lidar_cloud(1000000, seed=2)
        for slices in (1, 10):
            off = np.linspace(0, len(cur), slices + 1).astype(np.int64)
            ns = min(sum(ref_crop(lib, cur[off[s]:off[s + 1]], fx, fa)[3] for s in range(slices)) for _ in range(5))
            print(f"crop restated with the reference's computeBoundingBox + contains, {len(fx)} frame points against "
                  f"{slices} slice(s), one core: {ns / 1e6:.2f} ms")
    path = os.path.join(HERE, "ref_crop_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
