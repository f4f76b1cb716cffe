"""ctypes loader of tests/emu/libpred_repair_emu.so (TEST INFRASTRUCTURE): the predicting encoder with direct
predictors -- the library's passes, its ordered walk (pred_walk_kernel) and its host-side decisions
(csrc/pred_repair.hpp) -- compiled for the CPU wavefront emulator."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", EMU_DIR, "-f", "pred_repair.mk", "libpred_repair_emu.so"], check=True,
                       stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(EMU_DIR, "libpred_repair_emu.so"))
        _lib.pred_repair_emu_encode.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, C.c_void_p, _i32p,
                                                _i32p, C.c_void_p, C.c_int32, C.c_int32, _i32p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]
        _lib.pred_repair_emu_encode.restype = C.c_int
        _lib.pred_repair_emu_after_from_text.argtypes = [C.c_char_p]
        _lib.pred_repair_emu_after_from_text.restype = C.c_int
    return _lib


def after_from_text(text):
    """GPCC_PRED_REPAIR_AFTER as the library reads it"""
    return lib().pred_repair_emu_after_from_text(None if text is None else text.encode())


def encode(pp, lod, attrs, attrs_ref=None, repair_after=0, qp_off=None):
    """-> (values [n,c] coding order, recon [n,c] point order, icp int8 [32,3],
    dict(passes, differences, walked, stretches, longest_stretch, first, last: the first and last difference));
    repair_after 0: the library's default; qp_off [n, 2]: per-point QP offsets (point order)"""
    a = np.ascontiguousarray(attrs, dtype=np.int32).copy()
    n, c = a.shape
    v = np.zeros((n, c), np.int32)
    icp = np.zeros((32, 3), np.int8)
    stats = np.zeros(7, np.int64)
    ref = ar = None
    n_ref = 0
    if attrs_ref is not None:
        ref = np.ascontiguousarray(lod["ref"], dtype=np.int32).reshape(-1)
        ar = np.ascontiguousarray(attrs_ref, dtype=np.int32).reshape(-1)
        n_ref = len(ar)
    q = None if qp_off is None else np.ascontiguousarray(qp_off, dtype=np.int32)
    rc = lib().pred_repair_emu_encode(
        C.addressof(pp), n, c, np.ascontiguousarray(lod["nc"], dtype=np.int32),
        np.ascontiguousarray(lod["ni"], dtype=np.int32).reshape(-1),
        np.ascontiguousarray(np.asarray(lod["w"]).astype(np.int32)).reshape(-1),
        ref.ctypes.data if ref is not None else None, np.ascontiguousarray(lod["indexes"], dtype=np.int32),
        a.reshape(-1), ar.ctypes.data if ar is not None else None, n_ref, int(repair_after), v.reshape(-1),
        icp.ctypes.data, stats.ctypes.data, q.ctypes.data if q is not None else None)
    assert rc == 0, rc
    return v, a, icp, dict(zip(("passes", "differences", "walked", "stretches", "longest_stretch", "first", "last"),
                                (int(x) for x in stats)))
