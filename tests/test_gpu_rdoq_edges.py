"""The lossy encoder's RDOQ decision on the MI355X, piece by piece (exact comparisons only).

The reference keeps trainZeros as one loop-carried counter and zeroes a small coefficient when
(Dist2 << 26) < lambda * Rate(trainZeros) (tmc3/RAHT.cpp:1578-1669).  The library restates that as a threshold per
coefficient (rdoq_threshold / rdoq_threshold_recip, csrc/raht_levels.hpp: one double-precision quotient, two integer
repairs, a cap) and a parallel resolver of the carried state (rdoq_resolve_kernel, csrc/raht_rdoq.hpp: a fixed
point per 64-coefficient chunk, tiles of 2048 classified under two hypotheses, a decoupled look-back 64 words at a
time, slice_l from level to level).  Both run here on their own through gpcc_debug_rdoq_threshold and
gpcc_debug_rdoq_resolve:

* thresholds against the literal expression of the reference in exact integers, with d on both sides of every
  multiple of lambda up to the cap, for every lambda the quantiser can produce and for powers of two and their
  neighbours;
* the resolver against the sequential loop, on streams built to reach what natural data reaches by accident: chains
  of open tiles, windows that end exactly at a reset, thresholds longer than a tile, look-backs past 64 transparent
  tiles, levels that begin and end anywhere in a tile.  Which tiles are open / closed / transparent is computed from
  the loop alone (rdoq_cases.classify), and a case that does not reach what it is for fails."""
import ctypes as C

import numpy as np
import pytest

import rdoq_cases as rc

pytestmark = pytest.mark.gpu

_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def dev():
    from mpeg_pcc_tmc13_amd import _lib, context
    lib = _lib.load()
    lib.gpcc_debug_rdoq_threshold.restype = C.c_int
    lib.gpcc_debug_rdoq_threshold.argtypes = [C.c_void_p, _i64p, _i64p, _i32p, _u32p, C.c_int64, _u32p, _u32p]
    lib.gpcc_debug_rdoq_resolve.restype = C.c_int
    lib.gpcc_debug_rdoq_resolve.argtypes = [C.c_void_p, C.c_int32, _i64p, _i32p, _i32p, _u32p, C.c_int32, _i32p, _i32p]
    return lib, context(0)


# ---- thresholds -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold_cases(dev):
    d2, lam, rcf, lim = rc.threshold_inputs()
    assert 100_000 < len(d2) < 600_000, len(d2)
    lib, ctx = dev
    out_div, out_recip = np.zeros(len(d2), np.uint32), np.zeros(len(d2), np.uint32)
    assert lib.gpcc_debug_rdoq_threshold(ctx._h, d2, lam, rcf, lim, len(d2), out_div, out_recip) == 0, \
        lib.gpcc_last_error()
    return d2, lam, rcf, lim, {"division": out_div, "reciprocal": out_recip}


@pytest.mark.parametrize("which", ["division", "reciprocal"])
def test_threshold_decides_as_the_reference_expression(threshold_cases, which):
    d2, lam, rcf, lim, outs = threshold_cases
    rc.check_thresholds(d2, lam, rcf, lim, outs[which], which)


def test_threshold_cases_cover_what_they_are_for(threshold_cases):
    """(about the cases, not the library) both sides of the cap, every threshold value, and thresholds that meet
    their limit exactly"""
    d2, lam, rcf, lim, outs = threshold_cases
    rc.check_threshold_coverage(d2, lam, lim, outs["division"])


# ---- the resolver ---------------------------------------------------------------------------------------------
def _resolve(dev):
    lib, ctx = dev

    def call(offsets, cut_off, cuts, desc, c, coeffs):
        co = np.ascontiguousarray(coeffs, dtype=np.int32).copy()
        sl = np.full(len(offsets) - 1, -77, np.int32)
        cuts = cuts if len(cuts) else np.zeros(1, np.int32)
        code = lib.gpcc_debug_rdoq_resolve(ctx._h, len(offsets) - 1, offsets, cut_off, cuts,
                                           np.ascontiguousarray(desc, dtype=np.uint32), c, co, sl)
        assert code == 0, lib.gpcc_last_error()
        return co, sl
    return call


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("cuts", ["one_level", "seams"])
@pytest.mark.parametrize("broken", [False, True], ids=["chain", "broken"])
@pytest.mark.parametrize("thr", [1, 3, 9])
def test_domino(dev, thr, broken, cuts, c):
    d = rc.domino(thr, broken=broken)
    k = rc.CUTS[cuts](len(d))
    if cuts == "one_level":
        assert rc.open_tiles(d, k) >= 9
    zeroed, last = rc.reference(d, k)
    if broken:   # everything behind the candidate that lost its reset is zeroed
        p = 5 * rc.TILE + 1000
        assert last == p and zeroed[p + thr + 1:].all() and not zeroed[:p + 1].any()
    else:
        assert last == len(d) - 1 and not zeroed.any()
    rc.run_slices(_resolve(dev), [(d, k)], c, seed=thr)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("cuts", ["one_level", "seams"])
@pytest.mark.parametrize("placement", rc.EDGE_PLACEMENTS)
def test_edge_of_the_window(dev, placement, cuts, c):
    d, marks = rc.window_edge(placement)
    k = rc.CUTS[cuts](len(d))
    zeroed, _ = rc.reference(d, k)
    want = {"chunk": {1, 42}, "chunk_seam": {1, 1034}, "tile_seam": {1, 1034}, "tile_seam_late": {1, 1034},
            "two_tile_seams": {2058, 4106}}[placement]
    assert want <= {t for _, t, _ in marks}
    for p, thr, dist in marks:   # at distance thr the reset is still seen; one further it is not
        assert bool(zeroed[p + dist]) == (dist == thr + 1) and not zeroed[p]
    rc.run_slices(_resolve(dev), [(d, k)], c, seed=len(d))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("cuts", ["one_level", "early_seams"])
@pytest.mark.parametrize("case", rc.LOOKBACK_CASES)
def test_long_lookback(dev, case, cuts, c):
    d = rc.long_lookback(case)
    k = rc.CUTS[cuts](len(d))
    # an open tile behind >= 65 transparent ones of its level; the 262154 candidate of a 70-tile slice resets under
    # either hypothesis, so its tile is closed -- it walks back all the same (rdoq_cases.long_lookback)
    closed_by_construction = case in ("resets", "resets_no_reset")
    assert rc.longest_transparent_lookback(d, k, "OC" if closed_by_construction else "O") >= 65
    zeroed, last = rc.reference(d, k)
    p = (130 if case == "resets_open" else 68) * rc.TILE + 100
    if case.startswith("zeroed"):
        assert zeroed[p] and last == (-1 if case.endswith("_no_reset") else 5)
    else:
        assert not zeroed[p:p + 300].any() and last == p + 299
    rc.run_slices(_resolve(dev), [(d, k)], c, seed=7)


@pytest.mark.parametrize("c", [1, 3])
def test_slices(dev, c):
    slices = rc.slice_batch()
    assert len(slices) == 5 and len({len(k) for _, k in slices}) == 5
    assert rc.open_tiles(*slices[0]) >= 8
    rc.run_slices(_resolve(dev), list(slices), c, seed=2)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("cuts", ["one_level", "seams", "inner_seams"])
@pytest.mark.parametrize("shares", rc.MIXTURES, ids=lambda s: f"z{s[0]}-def{s[1]}")
def test_random_mixture(dev, shares, cuts, c):
    d = rc.mixture(*shares)
    k = rc.CUTS[cuts](len(d))
    zeroed, _ = rc.reference(d, k)
    cand = ((d >> 31) == 0) & ((d & rc.NEVER) != rc.NEVER) & (d != 0)
    inside = np.zeros(len(d), bool)
    inside[k[0]:k[-1]] = True
    assert (zeroed & cand).any() and (~zeroed & cand & inside).any()
    if shares == (0.97, 0.0005):
        assert rc.open_tiles(d, k) >= 3
    rc.run_slices(_resolve(dev), [(d, k)], c, seed=1)


def test_bad_level_ranges_are_refused(dev):
    """cuts outside the slice or not ascending never reach the kernel"""
    lib, ctx = dev
    off, cut_off = np.array([0, 10], np.int64), np.array([0, 2], np.int32)
    desc, co, sl = np.zeros(10, np.uint32), np.ones(10, np.int32), np.zeros(1, np.int32)
    for cuts in ([0, 11], [5, 5], [6, 2], [-1, 4]):
        assert lib.gpcc_debug_rdoq_resolve(ctx._h, 1, off, cut_off, np.array(cuts, np.int32), desc, 1, co, sl) == -1
    assert (co == 1).all()
