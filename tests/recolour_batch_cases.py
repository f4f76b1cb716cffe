"""Inputs and expectations shared by the tests of gpcc_dev_recolour_attrs (emulator, GPU): batches of slices in
gpcc_src_partition's layout -- `synth` clouds cut into slabs, each slab re-quantised into its own target -- and per
slice and attribute what recolour_attrs_cases.alone(...) gives for that slice BY ITSELF (the compiled reference where
oracle/_ref is built, else the oracle that tests/test_oracle_recolour.py pins to it).  Everything is made once per
process and left unchanged."""
import functools

import numpy as np

import recolour_attrs_cases as rac
from mpeg_pcc_tmc13_amd import recolour_params, synth

# the smallest shapes at which the forest can go wrong: a root that is a leaf (8, 10), one that goes straight to the
# subtree kernel (11 .. 1024), one that is split once first (1025 ..), slice boundaries inside a wavefront's
# 1024-position chunk of kd_minmax / kd_count and inside a 2048-entry scan block
EDGE_SIZES = (8, 10, 11, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)
# trees that end at different levels: the loop's "no node created" test is global
UNEVEN_SIZES = (12, 6000, 12)
# the most roots per point, two slices empty on both sides among them: pins the capacities re-derived for R roots
RAGGED_SIZES = tuple(int(v) for v in np.random.default_rng(40).integers(8, 601, 40))
RAGGED_SIZES = RAGGED_SIZES[:7] + (0,) + RAGGED_SIZES[7:29] + (0,) + RAGGED_SIZES[29:]
assert len(RAGGED_SIZES) == 42 and min(v for v in RAGGED_SIZES if v) >= 8 and RAGGED_SIZES.count(0) == 2


class Batch:
    """src_off / tgt_off int64 [S + 1], src_xyz / tgt_xyz int32 [., 3], attrs: four (values [ns, c], bitdepth) on the
    concatenated sources, offsets int32 [S, 3], scale"""

    def __init__(self, slices, scale, kind):
        self.scale, self.kind = scale, kind
        self.S = len(slices)
        self.src_off = np.cumsum([0] + [len(s[0]) for s in slices]).astype(np.int64)
        self.tgt_off = np.cumsum([0] + [len(s[1]) for s in slices]).astype(np.int64)
        self.src_xyz = np.ascontiguousarray(np.concatenate([s[0] for s in slices]), dtype=np.int32).reshape(-1, 3)
        self.tgt_xyz = np.ascontiguousarray(np.concatenate([s[1] for s in slices]), dtype=np.int32).reshape(-1, 3)
        self.offsets = np.ascontiguousarray([s[2] for s in slices], dtype=np.int32).reshape(-1, 3)
        ns = len(self.src_xyz)
        rng = np.random.default_rng(77)
        if kind == "lidar":
            a = np.concatenate([s[3] for s in slices]).astype(np.int32).reshape(ns, 1)
            pair = [(a, 8), (rng.integers(0, 256, (ns, 3)).astype(np.int32), 8)]
        else:
            a = np.concatenate([s[3] for s in slices]).astype(np.int32).reshape(ns, 3)
            pair = [(a, 8), (rng.integers(0, 1024, (ns, 1)).astype(np.int32), 10)]
        # colour, reflectance, colour + 9 mod 256, reflectance reversed WITHIN every slice's neighbours' reach
        self.attrs = [pair[0], pair[1], ((pair[0][0] + 9) % 256, pair[0][1]), (np.ascontiguousarray(pair[1][0][::-1]), pair[1][1])]
        for arr in (self.src_off, self.tgt_off, self.src_xyz, self.tgt_xyz, self.offsets, *[a for a, _ in self.attrs]):
            arr.setflags(write=False)
        # every non-empty slice has at least 8 source points and one target; only both sides may be empty
        for s in range(self.S):
            n_s, n_t = self.count(s)
            assert (n_s == 0 and n_t == 0) or (n_s >= 8 and n_t >= 1), (s, n_s, n_t)

    def count(self, s):
        return int(self.src_off[s + 1] - self.src_off[s]), int(self.tgt_off[s + 1] - self.tgt_off[s])

    def src(self, s):
        return slice(int(self.src_off[s]), int(self.src_off[s + 1]))

    def tgt(self, s):
        return slice(int(self.tgt_off[s]), int(self.tgt_off[s + 1]))

    @functools.lru_cache(maxsize=None)
    def want(self, kw_items, order):
        """-> per attribute of `order` the expected [nt, c]: every slice alone"""
        p = recolour_params(bitdepth=8, **dict(kw_items))
        out = []
        for i in order:
            a, depth = self.attrs[i]
            rows = [rac.alone(p, self.src_xyz[self.src(s)], a[self.src(s)], depth, self.tgt_xyz[self.tgt(s)], scale=self.scale,
                              offset=tuple(int(v) for v in self.offsets[s]))
                    for s in range(self.S) if self.count(s)[0]]
            w = np.concatenate(rows)
            w.setflags(write=False)
            out.append(w)
        return out


def target_of(xyz, scale, off):
    """requantise (tests/test_emu_recolour.py) with the slice's offset: posInTgt = posInSrc * scale - offset"""
    return np.unique(np.rint(xyz.astype(np.float64) * scale).astype(np.int32) - np.asarray(off, dtype=np.int32), axis=0)


@functools.lru_cache(maxsize=None)
def slabs(kind, sizes, seed=4):
    """a cloud cut along x into consecutive slabs of the given numbers of points -> [(xyz, attribute)]"""
    total = sum(sizes)
    if kind == "dense":
        xyz, a = synth.dense_cloud(2 * total + 2000, seed=seed, bits=7)
    else:
        xyz, a = synth.lidar_cloud(2 * total + 2000, seed=seed)
    assert len(xyz) >= total
    keep = np.sort(np.random.default_rng(seed).permutation(len(xyz))[:total])
    xyz, a = xyz[keep], a[keep]
    order = np.argsort(xyz[:, 0], kind="stable")
    xyz, a = xyz[order], a[order]
    cuts = np.cumsum((0,) + tuple(sizes))
    return [(xyz[cuts[i]:cuts[i + 1]], a[cuts[i]:cuts[i + 1]]) for i in range(len(sizes))]


@functools.lru_cache(maxsize=None)
def batch(kind, sizes, scale, vary_offsets=False):
    rng = np.random.default_rng(len(sizes))
    slices = []
    for i, (xyz, a) in enumerate(slabs(kind, tuple(sizes))):
        off = tuple(int(v) for v in rng.integers(-9, 10, 3)) if vary_offsets else (0, 0, 0)
        if vary_offsets and i == 0:
            off = (-7, 4, -1)
        tgt = target_of(xyz, scale, off) if len(xyz) else np.zeros((0, 3), np.int32)
        slices.append((xyz, tgt, off, a))
    return Batch(slices, scale, kind)


GEOM_LIMIT = 3.0


def kth_dist2(b, s, k):
    """squared distance of every target of slice s to its k-th nearest source point, in the source's frame"""
    q = (b.tgt_xyz[b.tgt(s)].astype(np.float64) + b.offsets[s]) * (1.0 / np.float64(np.float32(b.scale)))
    d = ((q[:, None, :] - b.src_xyz[b.src(s)].astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    return np.sort(d, axis=1)[:, k - 1]


@functools.lru_cache(maxsize=None)
def limit_batch():
    """three slices at scale 0.37 under max_geom_fwd = 3.0: the limit is reached in slices 0 and 2 (`dense`: sparse
    against the limit) but not in slice 1, whose sources sit on its own targets' positions -- eight of them, with
    different values, within 0.75 of every target's query point"""
    scale = 0.37
    (x0, a0), (x1, a1), (x2, a2) = slabs("dense", (1500, 900, 1300))
    t1 = target_of(x1, scale, (0, 0, 0))
    at = np.rint(t1.astype(np.float64) * (1.0 / np.float64(np.float32(scale)))).astype(np.int32)
    src1 = np.repeat(at, 8, axis=0)
    col1 = np.random.default_rng(5).integers(0, 256, (len(src1), 3)).astype(np.int32)
    slices = [(x0, target_of(x0, scale, (0, 0, 0)), (0, 0, 0), a0), (src1, t1, (0, 0, 0), col1),
              (x2, target_of(x2, scale, (2, -3, 1)), (2, -3, 1), a2)]
    return Batch(slices, scale, "dense")


def key(kw):
    return tuple(sorted(kw.items()))


def check(run, b, kw=None, order=(0, 1)):
    """`run(p, batch, attrs)` -> one [nt, c] array per attribute: exactly every slice's own result"""
    kw = kw or {}
    p = recolour_params(bitdepth=8, **kw)
    got = run(p, b, [b.attrs[i] for i in order])
    want = b.want(key(kw), tuple(order))
    assert len(got) == len(order)
    for g, w, i in zip(got, want, order):
        assert g.shape == w.shape
        for s in range(b.S):
            np.testing.assert_array_equal(g[b.tgt(s)], w[b.tgt(s)], err_msg=f"attribute {i}, slice {s} of {b.S}")
