"""TEST INFRASTRUCTURE: descriptor streams for rdoq_resolve_kernel (csrc/raht_rdoq.hpp), the sequential loop they
are checked against, and the classification of a tile that the loop alone gives.  Shared by
tests/test_gpu_rdoq_edges.py (the kernel on the MI355X) and tests/test_emu_rdoq.py (the same kernel under the CPU
wavefront emulator).

A descriptor is  z << 31 | thr:  z = every component quantises to 0, thr = the zero-run length from which the
coefficient is zeroed (NEVER: at no length).  The loop of tmc3/RAHT.cpp:1578-1669 in these terms, L the index of
the last reset:  tz = i - 1 - L;  zeroed = thr != NEVER and tz >= thr;  z or zeroed: the run goes on;  else L = i."""
import ctypes as C
import functools

import numpy as np

from oracle_loader import oracle

NEVER = 0x7FFFFFFF
ZERO = 0x80000000
TILE = 2048
WAVE = 64
# the values rdoq_threshold_of_quotient can give (NEVER apart)
THR_SET = [0, 1, 2, 3, 5, 7, 9] + [10 + (1 << (b - 1)) for b in range(1, 31)]
DEFINITE = NEVER           # not z, no threshold: always a reset
Z_KEEP = ZERO | NEVER      # z, never zeroed: the run goes on and the coefficient stays
Z_ZERO = ZERO              # z with threshold 0: the run goes on and the coefficient is zeroed


def resolve_loop(desc, a, b, L=-1, zeroed=None):
    """the sequential loop over [a, b) -> the last reset; zeroed [len(desc)] bool is filled in when given"""
    d = desc[a:b].tolist()
    for i, w in enumerate(d, a):
        thr = w & NEVER
        ze = thr != NEVER and i - 1 - L >= thr
        if ze and zeroed is not None:
            zeroed[i] = True
        if not (w >> 31 or ze):
            L = i
    return L


_memo = {}


def _memoised(kind, desc, key, compute):
    """the streams below are built once and read-only, so a result can be kept per stream (the entry holds the array:
    its id stays its own)"""
    k = (kind, id(desc)) + key
    if k not in _memo:
        _memo[k] = (desc, compute())
    return _memo[k][1]


def reference(desc, cuts):
    """-> (zeroed mask, final slice_l) of one slice whose levels are bounded by cuts (none: nothing is processed).
    Where the levels' seams lie does not matter to the loop: it runs from the first cut to the last."""
    if len(cuts) < 2:
        return np.zeros(len(desc), bool), -1

    def compute():
        zeroed = np.zeros(len(desc), bool)
        last = resolve_loop(desc, int(cuts[0]), int(cuts[-1]), -1, zeroed)
        zeroed.setflags(write=False)
        return zeroed, last
    return _memoised("ref", desc, (int(cuts[0]), int(cuts[-1])), compute)


def apply_reference(coeffs, zeroed):
    """coeffs [c, n] of one slice"""
    out = coeffs.copy()
    out[:, zeroed] = 0
    return out


def classify(desc, cuts):
    """per level, the tiles' kinds ('T' transparent, 'C' closed, 'O' open) from the loop alone: a tile is the part of
    a level inside one 2048-coefficient stretch counted from the slice's first coefficient.  The loop runs over
    the tile with L = -1 and with L = a - 1: the second run leaves L alone: transparent; both agree: closed."""
    def compute():
        levels = []
        for la, lb in zip(cuts[:-1], cuts[1:]):
            kinds = []
            for t in range(int(la) // TILE, (int(lb) - 1) // TILE + 1):
                a, b = max(t * TILE, int(la)), min((t + 1) * TILE, int(lb))
                old, recent = resolve_loop(desc, a, b, -1), resolve_loop(desc, a, b, a - 1)
                kinds.append("T" if recent == a - 1 else ("C" if old == recent else "O"))
            levels.append("".join(kinds))
        return levels
    return _memoised("kinds", desc, tuple(int(v) for v in cuts), compute)


def open_tiles(desc, cuts):
    return sum(k.count("O") for k in classify(desc, cuts))


def longest_transparent_lookback(desc, cuts, kinds_wanted="O"):
    """the largest number of transparent tiles directly in front of a tile of one of the wanted kinds, inside its
    level (-1: there is no such tile)"""
    best = -1
    for kinds in classify(desc, cuts):
        for t, k in enumerate(kinds):
            if k in kinds_wanted:
                best = max(best, t - len(kinds[:t].rstrip("T")))
    return best


def coefficients(n, c, seed):
    """arbitrary non-zero values: a zeroing that is missed and one that is wrong both show"""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 1000, (c, n)).astype(np.int32)
    return np.where(rng.random((c, n)) < 0.5, v, -v).astype(np.int32)


# ---- streams ------------------------------------------------------------------------------------------------
def _z_fill(n):
    d = np.full(n, Z_KEEP, np.uint32)
    d[1::2] = Z_ZERO
    return d


@functools.lru_cache(maxsize=None)
def domino(thr, tiles=10, broken=False):
    """a definite reset at 0, then candidates of one threshold only: each sees the reset in front of it, so every one
    resets in turn -- a chain through every chunk and every tile.  broken: one candidate in the middle of tile
    tiles // 2 sits at distance thr + 1 behind its reset (zero coefficients between), is zeroed, and with it every
    candidate after it."""
    n = tiles * TILE
    d = np.full(n, thr, np.uint32)
    d[0] = DEFINITE
    if broken:
        p = (tiles // 2) * TILE + 1000
        d[p + 1:p + thr + 1] = _z_fill(thr)
    d.setflags(write=False)
    return d


EDGE_THRESHOLDS = [t for t in THR_SET if 1 <= t <= 4106]
EDGE_PLACEMENTS = ["chunk", "chunk_seam", "tile_seam", "tile_seam_late", "two_tile_seams"]


@functools.lru_cache(maxsize=None)
def window_edge(placement, max_thr=4106):
    """per threshold two segments: a definite reset at p, zero coefficients, and ONE candidate at distance thr
    (it still sees the reset: it resets) or thr + 1 (it is zeroed).  placement says where the pair lies:
    inside one 64-coefficient chunk, across a chunk seam, across a tile seam (the candidate first in its tile, or
    the reset last in its tile), across two tile seams.
    -> (descriptors, [(p, thr, distance)])"""
    segs, marks, cur = [], [], 0
    for thr in EDGE_THRESHOLDS:
        if thr > max_thr:
            continue
        for dist in (thr, thr + 1):
            if placement == "chunk":
                if dist > WAVE - 1:
                    continue
                off = 3 * WAVE + (WAVE - 1 - dist)          # the candidate is the chunk's last lane
            elif placement == "chunk_seam":
                if dist > TILE - WAVE:
                    continue
                off = 5 * WAVE - 1 - (dist - 1) % WAVE      # the candidate is the first lane of a later chunk
            elif placement == "tile_seam":
                if dist > TILE:
                    continue
                off = TILE - dist                           # the candidate is the next tile's first coefficient
            elif placement == "tile_seam_late":
                if dist > TILE:
                    continue
                off = TILE - 1                              # the reset is the tile's last coefficient
            else:
                if dist <= TILE:
                    continue
                off = TILE - 9                              # 2058: two seams; 4106: three
            span = off + dist + 1
            length = -(-(span + 5) // TILE) * TILE
            d = _z_fill(length)
            d[off] = DEFINITE
            d[off + dist] = thr
            segs.append(d)
            marks.append((cur + off, thr, dist))
            cur += length
    d = np.concatenate(segs + [_z_fill(77)])
    d.setflags(write=False)
    return d, marks


LOOKBACK_CASES = ["zeroed", "resets", "zeroed_no_reset", "resets_no_reset", "resets_open"]


@functools.lru_cache(maxsize=None)
def long_lookback(case):
    """70 tiles + 500 coefficients, all z; a definite reset at 5 (absent in the *_no_reset cases) and in tile 68 one
    candidate whose threshold is shorter (131082: it is zeroed) or longer (262154: it resets, and the 299
    candidates of threshold 2 behind it follow) than the run in front of it.  Every tile but the level's first
    walks back for its incoming L, here past 67 transparent tiles.  With 131082 the tile is open as well (zeroed
    if nothing was ever reset, a reset if the tile's predecessor was one); with 262154 it cannot be: the threshold
    is longer than the slice, the candidate resets under either hypothesis and the tile is closed.
    resets_open is the open tile that RESETS: 131 tiles + 500, the definite reset at 4200 and the 262154 candidate
    in tile 130, 62139 coefficients inside its window, behind 127 transparent tiles."""
    if case == "resets_open":
        n, p = 131 * TILE + 500, 130 * TILE + 100
        d = _z_fill(n)
        d[4200] = DEFINITE
        d[p] = 262154
        d[p + 1:p + 300] = 2
        d.setflags(write=False)
        return d
    n = 70 * TILE + 500
    d = _z_fill(n)
    if not case.endswith("_no_reset"):
        d[5] = DEFINITE
    p = 68 * TILE + 100
    if case.startswith("resets"):
        d[p] = 262154
        d[p + 1:p + 300] = 2
    else:
        d[p] = 131082
    d.setflags(write=False)
    return d


MIXTURES = [(0.9, 0.002), (0.6, 0.01), (0.3, 0.05), (0.97, 0.0005)]


@functools.lru_cache(maxsize=None)
def mixture(z_share, def_share, n=40 * TILE + 77, seed=3):
    """seeded mixture: z with probability z_share, a definite reset with def_share, the rest candidates; the
    thresholds (of the z coefficients too) come from the real value set, short ones more often than long ones"""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    pool = np.array([t for t in THR_SET if t <= 131082] + [NEVER], np.uint32)
    # the index into the pool is the smaller of two draws: all values occur, the short ones more often
    k = np.minimum(rng.integers(0, len(pool), n), rng.integers(0, len(pool), n))
    d = pool[k]
    z = u < z_share
    d[z] |= ZERO
    d[(u >= z_share) & (u < z_share + def_share)] = DEFINITE
    d.setflags(write=False)
    return d


# ---- level cuts ---------------------------------------------------------------------------------------------
def one_level(n):
    return [0, n]


def seams(n):
    """levels of 1, 63, 64, 65, 2047, 2048 and 2049 coefficients, one that ends on a tile seam (8192), one that
    ends inside tile 4 and one wholly inside that tile (its first tile is its last, and the tile where the level
    before ended), the rest in one level -- as far as n reaches"""
    cuts = [0, 1, 64, 128, 193, 2240, 4288, 6337, 8192, 8892, 9192]
    cuts = [v for v in cuts if v < n]
    return cuts + [n]


def early_seams(n):
    """the small levels of seams(), then one level from the middle of tile 1 to the end: a long level that begins
    inside a tile"""
    return [v for v in [0, 1, 64, 128, 193, 2240, 2300] if v < n] + [n]


def inner_seams(n):
    """the first level begins behind the slice's first coefficient, the last ends before its last: what lies outside
    is not touched"""
    cuts = [7, 70, 2048 + 7, 3 * TILE, 3 * TILE + 1, 5 * TILE + 63, 17 * TILE - 1, 17 * TILE + 1, 30 * TILE]
    return [v for v in cuts if v < n - 3] + [n - 3]


CUTS = {"one_level": one_level, "seams": seams, "early_seams": early_seams, "inner_seams": inner_seams}


# ---- the 5-slice batch --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slice_batch(small=False):
    """-> [(descriptors, cuts)]: a domino slice next to an all-zero one, a slice of one coefficient, one without a
    processed level and a mixture; every slice has another number of levels"""
    dom = domino(3, tiles=3 if small else 10)
    zeros = np.full(3 * TILE + 5, Z_ZERO, np.uint32)
    one = np.array([5], np.uint32)              # a candidate with nothing in front of it: tz = 0, it resets
    idle = mixture(0.6, 0.01, n=100, seed=11)
    mix = mixture(0.9, 0.002, n=(2 if small else 5) * TILE + 77, seed=5)
    return [(dom, [0, 700, 2 * TILE + 1, len(dom)]), (zeros, [0, TILE + 3, len(zeros)]), (one, [0, 1]), (idle, []),
            (mix, [v for v in [0, 1, 64, 2049, 2 * TILE + 50] if v < len(mix)] + [len(mix)])]


def run_slices(resolve, slices, c, seed=0):
    """resolve(offsets, cut_off, cuts, desc, c, coeffs) -> (coeffs, slice_l): one call over the slices, compared
    exactly with the loop.  coeffs: the library's planar layout, slice s at offsets[s] * c, component k at k * n_s."""
    offsets = np.cumsum([0] + [len(d) for d, _ in slices]).astype(np.int64)
    cut_off = np.cumsum([0] + [len(k) for _, k in slices]).astype(np.int32)
    cuts = np.array([v for _, k in slices for v in k], np.int32)
    desc = np.concatenate([d for d, _ in slices]).astype(np.uint32)
    src = [coefficients(len(d), c, seed + 17 * s) for s, (d, _) in enumerate(slices)]
    got, got_l = resolve(offsets, cut_off, cuts, desc, c, np.concatenate([v.reshape(-1) for v in src]))
    for s, (d, k) in enumerate(slices):
        zeroed, want_l = reference(d, k)
        want = apply_reference(src[s], zeroed)
        g = got[offsets[s] * c:offsets[s + 1] * c].reshape(c, -1)
        bad = np.nonzero((g != want).any(axis=0))[0]
        assert bad.size == 0, (f"slice {s}: {bad.size} coefficients differ, first at {bad[:8].tolist()} "
                               f"(descriptors {[hex(int(x)) for x in d[bad[:8]]]})")
        assert int(got_l[s]) == want_l, (s, int(got_l[s]), want_l)


# ---- thresholds: rdoq_threshold / rdoq_threshold_recip (csrc/raht_levels.hpp) --------------------------------
LUT_BINS = [1, 2, 3, 5, 5, 7, 7, 9, 9, 11, 11]
RATE_COEFFS = [0, 256, 406, 512, 768, 3072]
LIMITS = [1, 5, 10, 11, 12, 13, 2057, 2058, 2059, 1 << 20, (1 << 31) - 2]
# trainZeros where Rate() steps, and one in front of each step
TRAIN_ZEROS = sorted(set(range(13)) | {10 + (1 << (b - 1)) - k for b in range(1, 31) for k in (0, 1)})
# RAHT quantisers: qp is clipped to [4, max_qp], max_qp = 51 + 6 (bitdepth - 8) with bitdepth <= 16
QP_RANGE = range(4, 51 + 6 * 8 + 1)


# Past the quantiser's largest lambda (35 * 14942208^2 < 2^53) the functions still claim an exact quotient while
# d < 2^63.  These are the lambdas a double no longer holds: 2^53 + 1 becomes 2^53, the quotient of d = k * 2^53
# comes out as k where the truth is just below k -- the only cases here in which the downward repair has work to
# do (below 2^53 both operands of the division are exact and its quotient is correctly rounded).
BEYOND = [(1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 54) - 1, (1 << 54) + 1, (1 << 55) - 1, (1 << 55) + 1]


def rate_bins(tz):
    """tmc3/RAHT.cpp:1619-1632, literally (the coefficients' own rate is added by the caller)"""
    rate = LUT_BINS[10 if tz > 10 else tz]
    if tz > 10:
        temp = tz - 11
        temp += 1
        a = 0
        while temp:
            a += 1
            temp >>= 1
        rate += 2 * a - 1
        rate += 2
    return rate


def lambdas():
    """-> (the quantiser's step sizes over the qp range, from the oracle; every lambda they give; 1 and the powers
    of two with their neighbours up to the largest of those)"""
    scale = oracle().fn("scale", C.c_int64, [C.c_int32, C.c_int64])
    steps = sorted({int(scale(qp, 1)) for qp in QP_RANGE})
    produced = sorted({l0 * l0 * f for l0 in steps for f in (25, 35)})
    pows, k = {1}, 1
    while (1 << k) - 1 <= produced[-1]:
        pows |= {v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v <= produced[-1]}
        k += 1
    return steps, produced, sorted(pows)


@functools.lru_cache(maxsize=None)
def threshold_inputs(stride=1):
    """-> dist2, lambda, rate_coeff, limit.  Every (lambda, m, side) is kept: dist2 = floor and ceil of
    m * lambda / 2^26 and one beyond each, m = 0 .. 129 (the cap is 128), so d lies on both sides of every multiple.
    The product with the 6 x 11 pairs (rate_coeff, limit) is thinned: the cases take the pairs in turn, one each,
    and six lambdas (1, the smallest and the largest produced, one of each factor, 2^33 - 1 and 2^33 + 1) take
    the full product.  BEYOND adds lambdas past the quantiser's range.  stride > 1 keeps every stride-th lambda
    outside those six."""
    steps, produced, pows = lambdas()
    mid = steps[len(steps) // 2]
    full = {1, produced[0], produced[-1], mid * mid * 25, mid * mid * 35, (1 << 33) - 1, (1 << 33) + 1}
    others = sorted((set(produced) | set(pows) | set(BEYOND)) - full)
    pairs = [(r, l) for r in RATE_COEFFS for l in LIMITS]
    d2, lam_, rc_, lim, turn = [], [], [], [], 0
    for lam in sorted(full | set(others[::stride])):
        around = set()
        for m in range(130):
            lo, hi = (m * lam) >> 26, -((-m * lam) >> 26)
            around |= {lo - 1, lo, hi, hi + 1}
        for d in sorted(v for v in around if v >= 0):
            for r, l in (pairs if lam in full else [pairs[turn % len(pairs)]]):
                d2.append(d), lam_.append(lam), rc_.append(r), lim.append(l)
            turn += 1
    return np.array(d2, np.int64), np.array(lam_, np.int64), np.array(rc_, np.int32), np.array(lim, np.uint32)


def check_thresholds(d2, lam, rcf, lim, thr, which):
    """thr is in the value set, and for every trainZeros <= limit it zeroes exactly when the reference's
    expression  (Dist2 << 26) < lambda * Rate  does.  A small threshold above the limit and NEVER behave alike."""
    assert np.isin(thr, np.array(THR_SET + [NEVER], np.uint32)).all(), np.unique(thr)
    # uint64 holds every product: dist2 << 26 < 130 lambda + 2^28 and Rate <= 11 + 61 + 12
    assert int(lam.max()) * 131 + (1 << 28) < 1 << 63
    d = d2.astype(np.uint64) << np.uint64(26)
    rate_c = ((rcf + 128) >> 8).astype(np.uint64)
    lamu = lam.astype(np.uint64)
    wrong = np.zeros(len(thr), bool)
    for tz in TRAIN_ZEROS:
        want = d < lamu * (np.uint64(rate_bins(tz)) + rate_c)
        got = (thr != NEVER) & (tz >= thr.astype(np.int64))
        wrong |= (want != got) & (tz <= lim.astype(np.int64))
    bad = np.nonzero(wrong)[0]
    assert bad.size == 0, (which, bad.size, [(int(d2[i]), int(lam[i]), int(rcf[i]), int(lim[i]), int(thr[i]))
                                             for i in bad[:5]])


def check_threshold_coverage(d2, lam, lim, thr):
    q = (d2.astype(object) << 26) // lam.astype(object)
    assert (q == 127).any() and (q == 128).any() and (q == 129).any()
    assert set(THR_SET) <= set(thr.tolist()), sorted(set(THR_SET) - set(thr.tolist()))
    assert ((thr == lim) & (thr > 10)).any()
