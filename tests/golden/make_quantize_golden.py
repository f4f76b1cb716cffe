#!/usr/bin/env python3
"""Generate tests/golden/quantize_golden.npz from the COMPILED REFERENCE: quantizePositions, quantizePositionsUniq and
samplePositionsUniq (pointset_processing.cpp:113-194, both unique forms through reducePointSet :53-103) over the
cases of tests/quantize_cases.py, and getPartition's walk (encoder.cpp:1611-1659) over every returned map.

The harness next to this file (quantize_harness.cpp) is compiled in a temporary directory together with the
reference's tmc3/pointset_processing.cpp, misc.cpp and tables.cpp where they lie; this runs only where the reference
tree exists.  Stored per case: the number of destination points and SHA-256 digests of the destination positions,
idxToSrcIdx, srcIdxDupList and the partition's source indices; for cases of at most FULL_MAX points the four arrays
in full as well.  Integer arrays and strings only.

Also stored, as a recorded result: the reference's time on one core of the machine this ran on (-O3, best of three)
for the 1 M-point sphere shell of quantize_cases.sphere_shell at scales 1, 0.5 and 0.125 (tools/quantize_time.py
prints it next to the device's), with the machine's name."""
import ctypes as C
import os
import platform
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import conftest  # noqa: E402,F401
import quantize_cases as qc  # noqa: E402

REF = os.environ.get("GPCC_REFERENCE", "/root/reference")
TIMED_SCALES = (1.0, 0.5, 0.125)
TIMED_POINTS = 1000000


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def build_harness(tmp, opt="-O2"):
    so = os.path.join(tmp, "libquantize_harness.so")
    tmc3 = os.path.join(REF, "tmc3")
    cmd = ["g++", opt, "-DNDEBUG", "-std=c++11", "-DTMC3_h", "-fPIC", "-shared", "-w", "-I" + tmc3,
           "-I" + os.path.join(REF, "dependencies", "nanoflann"), os.path.join(HERE, "quantize_harness.cpp"),
           os.path.join(tmc3, "pointset_processing.cpp"), os.path.join(tmc3, "misc.cpp"),
           os.path.join(tmc3, "tables.cpp"), "-o", so]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(so)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.quantize_ref.restype = C.c_int32
    lib.quantize_ref.argtypes = [C.c_int32, C.c_float, C.c_float, i32p, i32p, i32p, i32p, C.c_int32, i32p, i32p, i32p,
                                 i32p, C.POINTER(C.c_int64)]
    return lib


def ref_quantize(lib, c, mode=None):
    """-> (dst_xyz, idx_to_src, src_dup_next, partition source indices, nanoseconds)"""
    mode = c["mode"] if mode is None else mode
    assert qc.in_domain(c), "the reference's float -> int conversion is undefined for this case"
    src = c["src"]
    n = len(src)
    v = lambda t: np.array(t, np.int32)  # noqa: E731
    dst, idx, nxt, part = (np.zeros((n, 3), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32),
                           np.zeros(n, np.int32))
    ns = C.c_int64(0)
    k = lib.quantize_ref(mode, c["scale"], c["sample_scale"], v(c["offset"]), v(c["clamp_min"]), v(c["clamp_max"]),
                         src.reshape(-1), n, dst.reshape(-1), idx, nxt, part, C.byref(ns))
    return dst[:k].copy(), idx[:k].copy(), nxt, part, ns.value


def main():
    assert os.path.isdir(os.path.join(REF, "tmc3")), "the reference tree is needed to regenerate this fixture"
    out = {"names": np.array(qc.NAMES)}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_harness(tmp)
        for name in qc.NAMES:
            c = qc.case(name)
            dst, idx, nxt, part, _ = ref_quantize(lib, c)
            res = {"num_dst": np.int64(len(idx)), "dst_sha": np.array(qc.digest(dst)), "idx_sha": np.array(qc.digest(idx)),
                   "next_sha": np.array(qc.digest(nxt)), "part_sha": np.array(qc.digest(part))}
            if c["mode"] != 2:  # quantizePositions: the positions before merging
                res["keep_sha"] = np.array(qc.digest(ref_quantize(lib, c, mode=0)[0]))
            if len(c["src"]) <= qc.FULL_MAX:
                res.update(dst=dst, idx=idx, next=nxt, part=part)
            for k, v in res.items():
                out[f"{name}/{k}"] = v
            print(name, "points", len(c["src"]), "unique", len(idx))
        # what the tests of those names rely on
        assert out["edge/long_group/8193/num_dst"] == 8193 - 4097 + 1
        for name in ("m2_half", "m2_quarter", "wide_m2", "clamp_min", "clamp_max", "sub_rounds", "int_to_float"):
            assert out[f"{name}/num_dst"] < len(qc.case(name)["src"]), name
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_harness(tmp, "-O3")
        cloud = qc.sphere_shell(TIMED_POINTS)
        ms, uniq = [], []
        for s in TIMED_SCALES:
            c = qc._case(1, s, cloud, clamp=((0, 0, 0), (4095, 4095, 4095)))
            runs = [ref_quantize(lib, c) for _ in range(3)]
            ms.append(min(r[4] for r in runs) // 1000)
            uniq.append(len(runs[0][1]))
            out[f"timed/{s}/idx_sha"] = np.array(qc.digest(runs[0][1]))
            out[f"timed/{s}/next_sha"] = np.array(qc.digest(runs[0][2]))
            out[f"timed/{s}/dst_sha"] = np.array(qc.digest(runs[0][0]))
            print(f"quantizePositionsUniq, {TIMED_POINTS} points, scale {s}, one core: {ms[-1] / 1000:.1f} ms, "
                  f"{uniq[-1]} unique")
        out["timed/scales_x1000"] = np.array([int(s * 1000) for s in TIMED_SCALES], np.int64)
        out["timed/points"] = np.int64(TIMED_POINTS)
        out["timed/reference_us"] = np.array(ms, np.int64)
        out["timed/unique"] = np.array(uniq, np.int64)
        out["timed/machine"] = np.array(f"{cpu_name()}, one core, g++ -O3 -DNDEBUG")
    path = os.path.join(HERE, "quantize_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
