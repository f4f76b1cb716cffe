"""ctypes loader of tests/emu/libref_crop_emu.so (TEST INFRASTRUCTURE): the kernels of csrc/ref_crop.hpp compiled for
the CPU wavefront emulator with the flags of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "mpeg-pcc-tmc13_amd", "csrc")
SO = os.path.join(EMU_DIR, "libref_crop_emu.so")
SRCS = [os.path.join(EMU_DIR, "ref_crop_emu_harness.cpp"), os.path.join(EMU_DIR, "emu_core.cpp")]
# (tests/emu/Makefile: FLAGS)
FLAGS = ["-O1", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-variable", "-Wno-unused-but-set-variable",
         "-Wno-attributes", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-sign-compare",
         "-DGPCC_EXPERIMENTS=1", "-I" + EMU_DIR, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_lib = None


def _stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = SRCS + [os.path.join(CSRC, h) for h in ("ref_crop.hpp", "spherical.hpp", "recolour_kdtree.hpp",
                                                   "gpcc_primitives.hpp")]
    deps += [os.path.join(ROOT, "include", "gpcc_attr_mi355.h"), os.path.join(EMU_DIR, "hip", "hip_runtime.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def lib():
    global _lib
    if _lib is None:
        if _stale():
            subprocess.run([os.environ.get("CXX", "g++"), *FLAGS, "-shared", *SRCS, "-o", SO], check=True)
        _lib = C.CDLL(SO)
        _lib.ref_crop_emu.argtypes = [C.c_int32, _i64p, _i32p, C.c_int32, _i32p, _i32p, C.c_int32, _i32p, _i32p, C.c_int64,
                                      _i64p, _i32p, _i32p, C.c_int32]
        _lib.ref_crop_emu.restype = C.c_int
    return _lib


def ref_crop(xyz, offsets, frame_xyz, frame_attrs, capacity=None, misalign=0):
    """-> (return code, bounding boxes [slices, 6], ref_offsets [slices + 1], positions, attributes, the error word);
    return code 1: the capacity was too small and nothing was written"""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    fx = np.ascontiguousarray(frame_xyz, dtype=np.int32)
    fa = np.ascontiguousarray(frame_attrs, dtype=np.int32).reshape(len(fx), -1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    ns, c = len(offsets) - 1, fa.shape[1]
    cap = ns * len(fx) if capacity is None else int(capacity)
    ox, oa = np.full((max(cap, 1), 3), -1, np.int32), np.full((max(cap, 1), c), -1, np.int32)
    ro, bbox, err = np.zeros(ns + 1, np.int64), np.zeros((ns, 6), np.int32), np.zeros(1, np.int32)
    rc = lib().ref_crop_emu(ns, offsets, xyz.reshape(-1), len(fx), fx.reshape(-1), fa.reshape(-1), c, ox.reshape(-1),
                            oa.reshape(-1), cap, ro, bbox.reshape(-1), err, int(misalign))
    assert rc in (0, 1), rc
    k = 0 if rc else int(ro[-1])
    return rc, bbox, ro, ox[:k], oa[:k], int(err[0])
