"""Cases of the unique-position quantiser and the source partition (gpcc_quantize_positions, gpcc_src_partition),
shared by tests/golden/make_quantize_golden.py (the compiled reference), tests/test_quantize_golden.py (the NumPy
restatement below against the golden file), tests/test_emu_quantize.py (the kernels under the wavefront emulator) and
tests/test_gpu_quantize.py.  Inputs are generated, never stored: a case is its name.

The restatement: quantise() forms the reference's float expressions (pointset_processing.cpp:113-194) in float32;
reduce_point_set() is reducePointSet (:53-103) said with a stable sort; partition() is getPartition's walk
(encoder.cpp:1611-1659)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantize_golden.npz")
FULL_MAX = 300          # cases of at most this many points are stored in full, digests above
T = 4096                # the sort's tile (csrc/morton_sort.hpp kSortTile)
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]
PATTERNS = ["distinct", "identical", "doubled", "first_last", "tile_edge", "long_group", "rand30", "rand95"]
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
WIDE = ((INT_MIN,) * 3, (INT_MAX,) * 3)  # a clamp that never bites


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- inputs ----------------------------------------------------------------------------------------------------
def _distinct(rng, n, bits=12):
    """n different points of a 2^bits cube, in random order"""
    lin = rng.choice(1 << (3 * bits), size=n, replace=False) if n else np.zeros(0, np.int64)
    m = (1 << bits) - 1
    return np.stack([lin & m, (lin >> bits) & m, lin >> (2 * bits)], 1).astype(np.int32).reshape(n, 3)


def pattern_cloud(pattern, n, seed=0):
    """the duplicate patterns of the edge matrix on a 12-bit cloud (quantised at scale 1: equal points merge)"""
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + n + seed)
    if n == 0:
        return np.zeros((0, 3), np.int32)
    if pattern == "distinct":
        return _distinct(rng, n)
    if pattern == "identical":
        return np.repeat(_distinct(rng, 1), n, axis=0)
    if pattern == "doubled":  # source points i and i + 1 are equal
        return np.repeat(_distinct(rng, (n + 1) // 2), 2, axis=0)[:n].copy()
    if pattern == "first_last":
        p = _distinct(rng, n)
        p[-1] = p[0]
        return p
    if pattern == "tile_edge":  # a group of four around every multiple of the sort's tile
        p = _distinct(rng, n)
        for b in range(T, n, T):
            p[b - 2:min(n, b + 2)] = p[b - 2]
        return p
    if pattern == "long_group":  # more than half of the points are one point, spread over the cloud
        p = _distinct(rng, n)
        where = rng.choice(n, size=n // 2 + 1, replace=False)
        p[where] = p[where.min()]
        return p
    frac = {"rand30": 0.30, "rand95": 0.95}[pattern]
    pool = _distinct(rng, max(1, int(round(n * (1 - frac)))))
    p = np.concatenate([pool, pool[rng.integers(0, len(pool), n - len(pool))]]) if n > len(pool) else pool[:n]
    return p[rng.permutation(n)].copy()


def sphere_shell(n, bits=12, seed=1):
    """the measurement's cloud: n points on a sphere shell voxelised to `bits` bits, duplicates kept"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = 0.45 + 0.01 * rng.random((n, 1))
    return np.rint((0.5 + r * v) * ((1 << bits) - 1)).astype(np.int32)


def surface_cloud(n=3000, seed=5):
    """the end-to-end case: a 10-bit surface with colours, duplicates kept -> (xyz, colours)"""
    from mpeg_pcc_tmc13_amd import synth
    return synth.dense_cloud(n, seed=seed, bits=10, dedup=False)


def _signed(rng, n, mag, dup=0.3):
    p = rng.integers(-mag, mag + 1, (n, 3)).astype(np.int32)
    k = int(n * dup)
    p[rng.integers(0, n, k)] = p[rng.integers(0, n, k)]
    return p


def _case(mode, scale, src, offset=(0, 0, 0), clamp=WIDE, sample_scale=1.0):
    return {"mode": mode, "scale": scale, "sample_scale": sample_scale, "offset": tuple(offset),
            "clamp_min": tuple(clamp[0]), "clamp_max": tuple(clamp[1]), "src": np.ascontiguousarray(src, np.int32)}


def _arith(name):
    rng = np.random.default_rng(sum(name.encode()))
    n = 300
    if name == "half_away":  # odd coordinates of both signs at scale 0.5: -1.5 -> -2, 1.5 -> 2, 0.5 -> 1, -0.5 -> -1
        p = (2 * rng.integers(-40, 40, (n, 3)) + 1).astype(np.int32)
        return _case(1, 0.5, p)
    if name.startswith("scale_"):
        s = {"scale_0.3": 0.3, "scale_third": 1 / 3, "scale_1.7": 1.7, "scale_0.999999": 0.999999}[name]
        p = _signed(rng, n, 1 << 20)
        p[:40] = _signed(rng, 40, 8)   # a dense corner: merges
        return _case(1, s, p, offset=(-3, 5, 0))
    if name == "int_to_float":  # 2^24 + 1 is no float: int -> float rounds to even
        base = np.array([(1 << 24) + d for d in (-1, 0, 1, 2, 3, 5)] + [-(1 << 24) - 1, -(1 << 24) - 3], np.int32)
        return _case(1, 1.0, base[rng.integers(0, len(base), (n, 3))])
    if name == "sub_rounds":  # roundf(p * s) = 2^25 and offset -1: 2^25 + 1 is no float, the subtraction rounds
        base = np.array([(1 << 25) + d for d in (-4, -2, 0, 4, 8)], np.int32)
        return _case(1, 1.0, base[rng.integers(0, len(base), (n, 3))], offset=(-1, -1, -3))
    if name == "clamp_min":  # negative results clipped to 0: points that differed merge
        return _case(1, 0.5, _signed(rng, n, 20, dup=0), offset=(0, 0, 0), clamp=((0, 0, 0), (INT_MAX,) * 3))
    if name == "clamp_max":
        return _case(1, 1.0, _signed(rng, n, 50, dup=0), offset=(-10, 0, 10), clamp=((-20, -5, -60), (7, 7, 7)))
    if name == "wide_m1":  # 27 bits an axis: the two-round sort
        return _case(1, 1.0, _signed(rng, 2 * T + 1, 1 << 26, dup=0.5), offset=((1 << 25) + 1, 0, -7))
    if name == "wide_m2":  # negative keys in mode 2, spans above 2^22
        return _case(2, 0.5, _signed(rng, T + 1, 1 << 26, dup=0.5), offset=(9, -9, 1), sample_scale=0.25)
    if name == "full_int32":  # the whole int32 range on all three axes (2^31 - 128 is the largest float below 2^31)
        base = np.array([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 127, INT_MAX - 200], np.int32)
        return _case(1, 1.0, base[rng.integers(0, len(base), (n, 3))])
    if name == "m2_half":  # sample_scale / scale = 0.5: neighbours merge, the first one's position stays
        return _case(2, 1.0, _signed(rng, 1000, 30, dup=0.2), offset=(-4, 7, 100), sample_scale=0.5)
    if name == "m2_quarter":
        return _case(2, 0.5, _signed(rng, T + 1, 200, dup=0.2), offset=(3, 0, -3), sample_scale=0.125)
    if name == "m2_fine":  # a sampling grid finer than the quantiser's: only equal quantised points merge
        return _case(2, 0.3, _signed(rng, 500, 40, dup=0.1), sample_scale=0.6)
    if name == "surface_half":  # the end-to-end case of test_gpu_quantize.py
        return _case(1, 0.5, surface_cloud()[0], clamp=((0, 0, 0), (511, 511, 511)))
    raise KeyError(name)


ARITH = ["half_away", "scale_0.3", "scale_third", "scale_1.7", "scale_0.999999", "int_to_float", "sub_rounds",
         "clamp_min", "clamp_max", "wide_m1", "wide_m2", "full_int32", "m2_half", "m2_quarter", "m2_fine",
         "surface_half"]
MATRIX = [f"edge/{p}/{n}" for p in PATTERNS for n in SIZES]
NAMES = MATRIX + ARITH


def case(name):
    """-> dict(mode, scale, sample_scale, offset, clamp_min, clamp_max, src)"""
    if name.startswith("edge/"):
        _, pattern, n = name.split("/")
        return _case(1, 1.0, pattern_cloud(pattern, int(n)), clamp=((0, 0, 0), (4095, 4095, 4095)))
    return _arith(name)


# ---- the restatement -------------------------------------------------------------------------------------------
def _roundf(x):
    """std::round(float): halves away from zero (exact in float64, the result is a float32 again)"""
    x = x.astype(np.float64)
    return np.trunc(x + np.copysign(0.5, x)).astype(np.float32)


def in_domain(c):
    """every float the reference converts to int lies in [-2^31, 2^31)"""
    t = _roundf(c["src"].astype(np.float32) * np.float32(c["scale"]))
    if c["mode"] == 2:
        diff = np.float32(c["sample_scale"]) / np.float32(c["scale"])
        fs = [t, _roundf(t * diff)]
    else:
        fs = [t - np.asarray(c["offset"], np.int32).astype(np.float32)]
    return all(((f >= -2.0**31) & (f < 2.0**31)).all() for f in fs)


def quantise(c):
    """-> (keys int32 [n, 3], positions int32 [n, 3])"""
    src, s = c["src"], np.float32(c["scale"])
    t = _roundf(src.astype(np.float32) * s)            # int -> float32 rounds to nearest even
    off = np.asarray(c["offset"], np.int32)
    if c["mode"] == 2:
        diff = np.float32(c["sample_scale"]) / s       # a float division
        key = _roundf(t * diff).astype(np.int64)
        pos = t.astype(np.int64) - off                 # an integer subtraction, no clip
        return key.astype(np.int32), pos.astype(np.int32)
    f = t - off.astype(np.float32)                     # a float32 subtraction
    q = np.clip(f.astype(np.int64), np.asarray(c["clamp_min"], np.int64), np.asarray(c["clamp_max"], np.int64))
    return q.astype(np.int32), q.astype(np.int32)


def reduce_point_set(key, pos):
    """-> (dst_xyz [num_dst, 3], idx_to_src [num_dst], src_dup_next [n])"""
    n = len(key)
    idx = np.arange(n, dtype=np.int32)
    if n == 0:
        return pos.reshape(0, 3), idx, idx
    order = np.lexsort((idx, key[:, 2], key[:, 1], key[:, 0]))  # stable: ascending source index inside a group
    ks = key[order]
    same = (ks[1:] == ks[:-1]).all(axis=1)
    nxt = idx.copy()
    nxt[order[:-1][same]] = order[1:][same]
    head = np.ones(n, bool)
    head[order[1:][same]] = False
    idx_to_src = np.nonzero(head)[0].astype(np.int32)
    return np.ascontiguousarray(pos[idx_to_src]), idx_to_src, nxt.astype(np.int32)


def expected(c):
    """what gpcc_quantize_positions returns: mode 0 -> (positions, None, None)"""
    key, pos = quantise(c)
    if c["mode"] == 0:
        return pos, None, None
    return reduce_point_set(key, pos)


def partition(idx_to_src, nxt, indexes):
    """the source indices getPartition visits, in order"""
    m, nx, out = np.asarray(idx_to_src).tolist(), np.asarray(nxt).tolist(), []
    for d in np.asarray(indexes).tolist():
        s = m[d]
        while True:
            out.append(s)
            t = nx[s]
            if t == s:
                break
            s = t
    return np.array(out, np.int64)


def partition_slices(idx_to_src, nxt, indexes, index_offsets):
    """-> (source indices of all slices back to back, out_offsets int64 [S + 1])"""
    parts = [partition(idx_to_src, nxt, indexes[index_offsets[s]:index_offsets[s + 1]])
             for s in range(len(index_offsets) - 1)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), off


def index_lists(num_dst, seed=0):
    """per map: every destination index, a permuted list, a list with repeats"""
    rng = np.random.default_rng(seed + num_dst)
    every = np.arange(num_dst, dtype=np.int32)
    return {"all": every, "permuted": rng.permutation(every).astype(np.int32),
            "repeats": rng.integers(0, max(num_dst, 1), num_dst // 2 + 3).astype(np.int32) if num_dst else every}


def ragged_slices(num_dst, slices=300, seed=3):
    """300 ragged slices, empty ones included -> (indexes, index_offsets int32 [slices + 1])"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 40, slices)
    sizes[rng.integers(0, slices, slices // 10)] = 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return rng.integers(0, num_dst, int(off[-1])).astype(np.int32), off


# ---- the golden file -------------------------------------------------------------------------------------------
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = np.load(GOLDEN)
    return _golden


def check_against_golden(name, dst, idx, nxt, what=""):
    """the three outputs (and the partition of every destination index) against the stored reference result"""
    g = golden()
    assert int(g[f"{name}/num_dst"]) == len(idx), (name, what)
    assert str(g[f"{name}/dst_sha"]) == digest(np.asarray(dst, np.int32)), (name, what, "positions")
    assert str(g[f"{name}/idx_sha"]) == digest(np.asarray(idx, np.int32)), (name, what, "idx_to_src")
    assert str(g[f"{name}/next_sha"]) == digest(np.asarray(nxt, np.int32)), (name, what, "src_dup_next")
    if f"{name}/dst" in g.files:
        np.testing.assert_array_equal(dst, g[f"{name}/dst"])
        np.testing.assert_array_equal(idx, g[f"{name}/idx"])
        np.testing.assert_array_equal(nxt, g[f"{name}/next"])
