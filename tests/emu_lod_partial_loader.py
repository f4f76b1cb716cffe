"""ctypes loader of tests/emu/liblod_partial_emu.so (TEST INFRASTRUCTURE): the scalable-lifting LoD
build of a partially decoded slice (lod_scalable.hpp with a first level and a skipped-point count)
and the quantisation weights of such a slice, compiled for the CPU wavefront emulator with the flags
of tests/emu/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "mpeg-pcc-tmc13_amd", "csrc")
SO = os.path.join(EMU_DIR, "liblod_partial_emu.so")
SRCS = [os.path.join(EMU_DIR, "lod_partial_emu_harness.cpp"), os.path.join(EMU_DIR, "emu_core.cpp")]
# (tests/emu/Makefile: FLAGS)
FLAGS = ["-O1", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-variable", "-Wno-unused-but-set-variable",
         "-Wno-attributes", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-sign-compare",
         "-DGPCC_EXPERIMENTS=1", "-I" + EMU_DIR, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_lib = None


def _stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = SRCS + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.startswith(("lod_", "lift_"))]
    deps += [os.path.join(ROOT, "include", "gpcc_attr_mi355.h"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
             os.path.join(EMU_DIR, "lod_emu_blocks.hpp")]
    return any(os.path.getmtime(d) > t for d in deps)


def lib():
    global _lib
    if _lib is None:
        if _stale():
            subprocess.run([os.environ.get("CXX", "g++"), *FLAGS, "-shared", *SRCS, "-o", SO], check=True)
        _lib = C.CDLL(SO)
        _lib.lod_emu_partial_build.argtypes = [C.c_void_p, _i32p, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p,
                                               _i32p, _i32p, C.POINTER(C.c_int32)]
        _lib.lod_emu_partial_build.restype = C.c_int
        _lib.quant_weights_emu_partial.argtypes = [C.c_int32, C.c_int32, C.c_int32, _i32p, C.c_int32, _u64p]
        _lib.quant_weights_emu_partial.restype = C.c_int
    return _lib


def partial_build(lp, xyz, min_geom_node_size_log2, geom_num_points):
    """-> dict as Context.lod_build(..., min_geom_node_size_log2, geom_num_points)"""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    n = len(xyz)
    nc = np.zeros(n, np.int32)
    ni = np.zeros((n, 3), np.int32)
    w = np.zeros((n, 3), np.int32)
    idx = np.zeros(n, np.int32)
    npl = np.zeros(32, np.int32)
    nl = C.c_int32()
    rc = lib().lod_emu_partial_build(C.addressof(lp), xyz.reshape(-1), n, int(min_geom_node_size_log2),
                                     int(geom_num_points), nc, ni.reshape(-1), w.reshape(-1), idx, npl, C.byref(nl))
    assert rc == 0, rc
    return dict(nc=nc, ni=ni, w=w, indexes=idx, npl=npl[:nl.value].copy())


def quant_weights(n, min_geom_node_size_log2, geom_num_points, npl):
    """the device's quantisation weights of a partially decoded scalable-lifting slice -> uint64 [n]"""
    qw = np.zeros(n, np.uint64)
    npl = np.ascontiguousarray(npl, dtype=np.int32)
    rc = lib().quant_weights_emu_partial(n, int(min_geom_node_size_log2), int(geom_num_points), npl, len(npl), qw)
    assert rc == 0, rc
    return qw
