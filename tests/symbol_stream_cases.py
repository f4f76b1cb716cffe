"""TEST INFRASTRUCTURE shared by tests/test_emu_symbol_stream.py and tests/test_gpu_dev_symbols.py: the edge matrix of
the device tier's entropy front end (csrc/symbol_stream.hpp), its expected results from the C oracle, slice by slice,
and the ctypes loader of tests/emu/libsymbol_stream_emu.so."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import lod_helpers as lh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

T = 1024  # kSymTile: positions per workgroup
W = 64    # the wavefront
INT32_MAX = 2**31 - 1
LENGTHS = [1, 2, W - 1, W, W + 1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3]
PATTERNS = ["all_zero", "no_zero", "first_only", "last_only", "tile_edge", "empty_tiles", "alternating", "rand0.001",
            "rand0.5", "rand0.999"]
# (the constants of ZR_PALETTE in tests/test_entropy_front_edges.py)
ZR_PALETTE = np.array([1, -1, INT32_MAX, -INT32_MAX, 2, -3, 70000, -(1 << 20), 255, -256, 1 << 30], np.int32)
# the class edges of bins_run_length and bins_symbol
RUN_EDGES = [0, 1, 2, 3, 4, 10, 11, 12, 13, 1 << 20]
MAG_EDGES = [1, 2, 3, 4, 7, 8, 1 << 30, INT32_MAX]


def positions(pattern, n):
    """sorted positions of the coded (not all-zero) points of a stream of n"""
    if pattern == "all_zero":
        return np.zeros(0, np.int64)
    if pattern == "no_zero":
        return np.arange(n)
    if pattern == "first_only":
        return np.array([0])
    if pattern == "last_only":
        return np.array([n - 1])
    if pattern == "tile_edge":
        # exactly the last position of a tile and the first of the next (what of them the stream has)
        return np.array([p for p in (T - 1, T) if p < n] or [n - 1])
    if pattern == "empty_tiles":
        # one run over three whole tiles without a coded position (tiles 1 .. 3), between two coded positions
        return np.unique(np.minimum(np.array([5, 4 * T + 1]), n - 1))
    if pattern == "alternating":
        return np.arange((n - 1) % 2, n, 2)
    density = float(pattern[4:])
    rng = np.random.default_rng([n, int(density * 1000)])
    return np.flatnonzero(rng.random(n) < density)


def stream(pattern, n, c, mode="mixed", shift=0):
    """the logical stream [n, c]: palette values at the pattern's positions.  c == 3, mode "mixed": the set of
    non-zero components cycles through all seven non-empty sets; "single": exactly one component is non-zero"""
    pos = positions(pattern, n)
    k = np.arange(len(pos)) + shift
    d = np.arange(c)
    vals = ZR_PALETTE[(k[:, None] + 4 * d[None, :]) % len(ZR_PALETTE)]
    if c > 1:
        if mode == "single":
            keep = d[None, :] == (k % c)[:, None]
        else:
            keep = (((1 + k % ((1 << c) - 1))[:, None] >> d[None, :]) & 1) != 0
        vals = np.where(keep, vals, 0).astype(np.int32)
    out = np.zeros((n, c), np.int32)
    out[pos] = vals
    return out


def stream_of_symbols(runs, values, trailing):
    """the logical stream [n, c] that has these symbols"""
    runs = np.asarray(runs, np.int64)
    values = np.asarray(values, np.int32).reshape(len(runs), -1)
    pos = np.cumsum(runs + 1) - 1
    n = int(pos[-1] + 1 if len(pos) else 0) + int(trailing)
    out = np.zeros((n, values.shape[1]), np.int32)
    out[pos] = values
    return out


def modes(c):
    return ("mixed", "single") if c == 3 else ("mixed",)


def pack_batch(slices, planar):
    """slices: logical streams [n_s, c] -> (offsets, the batch's coefficients flat, slice s at c * offsets[s])"""
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in slices])]).astype(np.int64)
    flat = np.concatenate([(np.ascontiguousarray(s.T) if planar else s).reshape(-1) for s in slices]).astype(np.int32)
    return offsets, flat


def unpack_batch(flat, offsets, c, planar):
    """the logical streams of a batch's coefficients"""
    out = []
    for s in range(len(offsets) - 1):
        b, e = int(offsets[s]), int(offsets[s + 1])
        part = flat[c * b:c * e]
        out.append(part.reshape(c, e - b).T if planar else part.reshape(e - b, c))
    return out


_expected = {}


def expected(logical):
    """(runs, values, trailing run, bins) of one slice from the C oracle; computed once per stream, never changed"""
    logical = np.ascontiguousarray(logical, dtype=np.int32)
    key = (logical.shape, hashlib.sha1(logical.tobytes()).digest())
    if key in _expected:
        return _expected[key]
    n, c = logical.shape
    runs, values, trailing = lh.oracle_zero_run_pack(logical, n, c, False)
    bins = lh.oracle_binarise_symbols(runs, values, trailing, c)
    for a in (runs, values, bins):
        a.setflags(write=False)
    _expected[key] = (runs, values, trailing, bins)
    return runs, values, trailing, bins


def check_batch(slices, got, what, symbols=True):
    """got: (bin_offsets, num_symbols, trailing_run, bins, runs or None, values or None) of a batch against the oracle,
    slice by slice; runs [n], values [n, c] as the entry lays them out"""
    bo, nsym, trail, bins, runs, values = got
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in slices])])
    assert bo[0] == 0, what
    for s, logical in enumerate(slices):
        er, ev, et, eb = expected(logical)
        b = int(offsets[s])
        assert nsym[s] == len(er), (what, s, "number of symbols", nsym[s], len(er))
        assert trail[s] == et, (what, s, "trailing run", trail[s], et)
        assert bo[s + 1] - bo[s] == len(eb), (what, s, "number of bins", bo[s + 1] - bo[s], len(eb))
        np.testing.assert_array_equal(bins[bo[s]:bo[s + 1]], eb, err_msg=f"{what}: bins of slice {s}")
        if symbols:
            np.testing.assert_array_equal(runs[b:b + len(er)], er, err_msg=f"{what}: runs of slice {s}")
            np.testing.assert_array_equal(values[b:b + len(er)], ev, err_msg=f"{what}: values of slice {s}")


# ---- the CPU wavefront emulator ----------------------------------------------------------------------------------
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", EMU_DIR, "-f", "symbol_stream.mk", "libsymbol_stream_emu.so"], check=True,
                       stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(EMU_DIR, "libsymbol_stream_emu.so"))
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        _lib.symbol_stream_emu_bins.argtypes = [i32, vp, vp, i32, i32, vp, i64, vp, vp, vp, vp, vp]
        _lib.symbol_stream_emu_unpack.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, vp]
    return _lib


def emu_bins(slices, planar, symbols=True, capacity=None):
    """-> (rc, (bin_offsets, num_symbols, trailing_run, bins, runs, values)); capacity None: sized by a first call"""
    c = slices[0].shape[1]
    offsets, flat = pack_batch(slices, planar)
    ns, n = len(slices), int(offsets[-1])
    bo = np.full(ns + 1, -1, np.int64)
    nsym, trail = np.full(ns, -1, np.int32), np.full(ns, -1, np.int32)
    runs = np.zeros(n, np.int32) if symbols else None
    values = np.zeros((n, c), np.int32) if symbols else None

    def call(bins):
        return emu().symbol_stream_emu_bins(
            ns, offsets.ctypes.data, flat.ctypes.data, c, int(planar), bins.ctypes.data, len(bins), bo.ctypes.data,
            runs.ctypes.data if symbols else None, values.ctypes.data if symbols else None, nsym.ctypes.data,
            trail.ctypes.data)
    if capacity is None:
        rc = call(np.zeros(0, np.uint8))
        assert rc in (0, 1), rc
        capacity = int(bo[ns])
    bins = np.full(capacity, 0xEE, np.uint8)
    rc = call(bins)
    return rc, (bo, nsym, trail, bins, runs, values)


def emu_unpack(lengths, symbols, c, planar):
    """symbols: per slice (runs, values) -> (rc, error word, the batch's coefficients flat)"""
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    so = np.concatenate([[0], np.cumsum([len(r) for r, _ in symbols])]).astype(np.int64)
    runs = np.concatenate([np.asarray(r, np.int32) for r, _ in symbols] + [np.zeros(1, np.int32)])
    values = np.concatenate([np.asarray(v, np.int32).reshape(-1) for _, v in symbols] + [np.zeros(c, np.int32)])
    out = np.full(c * int(offsets[-1]), 0x5A5A5A5A, np.int32)
    err = np.zeros(1, np.int32)
    rc = emu().symbol_stream_emu_unpack(len(lengths), offsets.ctypes.data, so.ctypes.data, runs.ctypes.data,
                                        values.ctypes.data, out.ctypes.data, c, int(planar), err.ctypes.data)
    return rc, int(err[0]), out
