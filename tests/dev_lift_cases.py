"""TEST INFRASTRUCTURE shared by tests/test_emu_lift_batch.py and tests/test_gpu_dev_lift.py: the case table of the
device tier's lifting transform over a held LoD structure (gpcc_dev_lift_forward / _inverse, csrc/lift_batch.hpp),
its expected results from the C oracle slice by slice (the oracle's lifting over the oracle's LoD structure,
lod_helpers; computed once, never changed), and the ctypes loader of tests/emu/liblift_batch_emu.so.

Batches (clouds: synth.dense_cloud, seeds 300.., 4-bit coordinates below 1 000 points, 9-bit above):
  "distance"  distance decimation (lod_params()), slices of 1, 2, 7, 63, 64, 65, 255, 257, 4097 and 20 points in ONE
              batch: a slice without any step ([1]), empty LoDs ([1, 2, 2], [1, 3, 5, 7, 7]), four different level
              counts (1, 3, 5, 10), steps in which a single slice works
  "ragged"    the same decimation, 300 slices of 1..40 points
  "periodic"  lod_params(levels=4, decimation=1): exactly 4 levels whatever the size ([1, 1, 1, 1] for one point)
Per slice the parameter blocks differ (QP, a second QP layer on every fourth slice), so a slice that read its
neighbour's block would show."""
import ctypes as C
import os
import subprocess

import numpy as np

import dev_raht_attr_cases as dc
import lod_helpers as lh
import oracle_loader as ol
from mpeg_pcc_tmc13_amd import lod_params, synth
from mpeg_pcc_tmc13_amd.params import LiftParams, lift_params_of_lod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

DIST_SIZES = [1, 2, 7, 63, 64, 65, 255, 257, 4097, 20]
BASE_QP = {8: 31, 10: 40, 16: 58}
# (c, LCP flag, bit depth): c in 1 and 3, the flag on and off, depths 8 and 16
CONFIGS = [(1, False, 8), (3, True, 8), (3, False, 8), (1, False, 16), (3, True, 16)]
MODES = ("plain", "regions", "scalable")


def sizes(batch):
    if batch == "distance":
        return list(DIST_SIZES)
    if batch == "ragged":
        return [int(v) for v in np.random.default_rng(300).integers(1, 41, 300)]
    raise KeyError(batch)


def coord_bits(n):
    return 4 if n < 1000 else 9


def lod_params_of(batch):
    return lod_params(levels=4, decimation=1) if batch == "periodic" else lod_params()


def faces_box(bits):
    """one box well inside the cube (dense_cloud's shells leave the outermost cells of a 4-bit cube empty): the
    255-point slice has points on each of its six faces, inside it and outside it (asserted by the GPU test)"""
    lo = 3 << (bits - 4)
    return [((lo,) * 3, ((1 << bits) - 1 - lo,) * 3, (3, -2))]


def overlap_boxes(bits):
    """two boxes that share a slab through the middle of the cube (the clouds are shells: a shared CORNER at the
    centre would hold no point), different offsets: the first wins there"""
    top, h, unit = (1 << bits) - 1, 1 << (bits - 1), 1 << (bits - 4)
    return [((0, 0, 0), (top, top, h + unit), (-3, 1)), ((0, 0, h - 2 * unit), (top, top, top), (4, -4))]


def boxes_of(batch, s, n):
    """the QP region boxes of slice s in mode "regions" ([]: none)"""
    bits = coord_bits(n)
    if batch == "distance":
        kind = {1: "all", 20: "faces", 255: "faces", 257: "overlap", 4097: "eight"}.get(n)
    else:
        kind = "overlap" if s % 7 == 3 else ("eight" if s % 11 == 5 else ("faces" if s % 13 == 1 else None))
    if kind == "all":
        return [((0, 0, 0), ((1 << bits) - 1,) * 3, (2, -1))]
    if kind == "faces":
        return faces_box(bits)
    if kind == "overlap":
        return overlap_boxes(bits)
    if kind == "eight":
        return dc.eight_boxes(bits)
    return []


class Batch:
    """offsets, xyz [N, 3] and colours [N, 3] in point order, and per slice the oracle's LoD structure"""

    def __init__(self, name, slice_sizes=None, seed=300):
        self.name = name
        self.lengths = sizes(name) if slice_sizes is None else [int(v) for v in slice_sizes]
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        lp = lod_params_of(name)
        xyz, col, self.lods = [], [], []
        for k, n in enumerate(self.lengths):
            x, a = synth.dense_cloud(n, seed=seed + k, bits=coord_bits(n))
            assert len(x) == n
            xyz.append(x.astype(np.int32))
            col.append(a.astype(np.int32))
            self.lods.append(lh.oracle_lod_generate(x, lp))
        self.xyz = np.concatenate(xyz)
        self.colour = np.concatenate(col)
        self.npl = [[int(v) for v in lod["npl"]] for lod in self.lods]
        for a in (self.xyz, self.colour, self.offsets):
            a.setflags(write=False)

    def slice(self, a, s):
        return a[int(self.offsets[s]):int(self.offsets[s + 1])]

    def attrs(self, c, bitdepth):
        """[N, c]: the cloud's colours scaled to the bit depth"""
        return np.ascontiguousarray(self.colour[:, :c] << (bitdepth - 8)).astype(np.int32)

    def structure(self):
        """the batch's structure as gpcc_dev_lod_build leaves it: (count [N], index [N, 3], weight [N, 3], indexes [N])"""
        return (np.concatenate([l["nc"] for l in self.lods]).astype(np.int32),
                np.concatenate([l["ni"] for l in self.lods]).astype(np.int32),
                np.concatenate([l["w"].astype(np.int32) for l in self.lods]),
                np.concatenate([l["indexes"] for l in self.lods]).astype(np.int32))

    def params(self, c, lcp, bitdepth, mode="plain", npl=None):
        """one LiftParams per slice"""
        out = []
        for s, n in enumerate(self.lengths):
            qp = BASE_QP[bitdepth] + 3 * (s % 3)
            chroma = -1 if c == 3 else 0
            layers = [(qp, chroma), (qp + 5, 1 if c == 3 else 0)] if s % 4 == 1 else None
            out.append(lift_params_of_lod(
                (npl or self.npl)[s], regions=boxes_of(self.name, s, n) if mode == "regions" else None, qp=qp,
                chroma_offset=chroma, bitdepth=bitdepth, lcp=lcp, layers=layers,
                scalable=(mode == "scalable" and s % 2 == 0)))
        return out

    def region_offsets(self, s, mode):
        """[n_s, 2] by point, what gpcc_lift_forward takes as qp_off; None: the slice names no region"""
        boxes = boxes_of(self.name, s, self.lengths[s]) if mode == "regions" else []
        return dc.region_offsets(self.slice(self.xyz, s), boxes) if boxes else None


_batches = {}


def batch(name):
    if name not in _batches:
        _batches[name] = Batch(name)
    return _batches[name]


# ---- expected results: the C oracle, slice by slice ----------------------------------------------------------------
_expected = {}


def expected(name, c, lcp, bitdepth, mode="plain"):
    """-> per slice (coeffs [n, c] coding order, reconstruction [n, c] point order, lcp int8 [32])"""
    key = (name, c, lcp, bitdepth, mode)
    if key not in _expected:
        b = batch(name)
        attrs = b.attrs(c, bitdepth)
        out = []
        for s, p in enumerate(b.params(c, lcp, bitdepth, mode)):
            co, rec, l = lh.lift(ol.oracle(), True, p, b.lods[s], b.slice(attrs, s), qp_off=b.region_offsets(s, mode))
            inv = lh.lift(ol.oracle(), False, p, b.lods[s], rec, coeffs=co, lcp=l, qp_off=b.region_offsets(s, mode))[1]
            np.testing.assert_array_equal(inv, rec)   # (the oracle's decoder reproduces its encoder)
            for a in (co, rec, l):
                a.setflags(write=False)
            out.append((co, rec, l))
        _expected[key] = out
    return _expected[key]


# ---- the CPU wavefront emulator ----------------------------------------------------------------------------------
_lib = None
PATTERN = 0x5A5A5A5A


def emu():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", EMU_DIR, "-f", "lift_batch.mk", "liblift_batch_emu.so"], check=True,
                       stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(EMU_DIR, "liblift_batch_emu.so"))
        vp, i32 = C.c_void_p, C.c_int32
        _lib.lift_batch_emu.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return _lib


def emu_lift(forward, params_list, offsets, structure, c, attrs=None, coeffs=None, lcp=None, xyz=None):
    """-> (rc, verdict, launches, attrs [N, c], coeffs [N, c], lcp int8 [S, 32]); an array the call only writes
    starts as PATTERN (lcp: 0x5A)"""
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    s, n = len(offs) - 1, int(offs[-1])
    arr = (LiftParams * s)(*params_list)
    nc, ni, nw, ix = (np.ascontiguousarray(a, dtype=np.int32) for a in structure)
    a = np.full((n, c), PATTERN, np.int32) if attrs is None else np.ascontiguousarray(attrs, dtype=np.int32).copy()
    co = np.full((n, c), PATTERN, np.int32) if coeffs is None else np.ascontiguousarray(coeffs, dtype=np.int32).copy()
    l = np.full((s, 32), 0x5A, np.int8) if lcp is None else np.ascontiguousarray(lcp, dtype=np.int8).copy()
    x = None if xyz is None else np.ascontiguousarray(xyz, dtype=np.int32)
    verdict, launches = C.c_int32(-1), C.c_int32(-1)
    rcode = emu().lift_batch_emu(
        C.addressof(arr), s, offs.ctypes.data, c, int(forward), nc.ctypes.data, ni.ctypes.data, nw.ctypes.data,
        ix.ctypes.data, None if x is None else x.ctypes.data, a.ctypes.data, co.ctypes.data, l.ctypes.data,
        C.addressof(verdict), C.addressof(launches))
    return rcode, verdict.value, launches.value, a, co, l
