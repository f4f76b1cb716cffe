"""rdoq_resolve_kernel and the RDOQ threshold functions under the CPU wavefront emulator (no GPU): the streams, the
sequential loop and the tile classification of tests/rdoq_cases.py, as tests/test_gpu_rdoq_edges.py runs them on the
device -- sizes cut where a chain of 64 fixed-point rounds per chunk costs the emulator seconds, the look-back past
64 transparent tiles kept.  A fault suspected in the resolver is looked for here, with gdb on this build."""
import numpy as np
import pytest

import emu_rdoq_loader as emu
import rdoq_cases as rc


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("broken", [False, True], ids=["chain", "broken"])
@pytest.mark.parametrize("thr,tiles", [(1, 4), (3, 10), (9, 10)])
def test_domino(thr, tiles, broken, c):
    d = rc.domino(thr, tiles=tiles, broken=broken)
    k = rc.one_level(len(d))
    assert rc.open_tiles(d, k) >= tiles - 1
    zeroed, last = rc.reference(d, k)
    assert last == ((tiles // 2) * rc.TILE + 1000 if broken else len(d) - 1) and zeroed.any() == broken
    rc.run_slices(emu.resolve, [(d, k)], c, seed=thr)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("placement", rc.EDGE_PLACEMENTS)
def test_edge_of_the_window(placement, c):
    d, marks = rc.window_edge(placement, max_thr=2058)
    k = rc.one_level(len(d))
    zeroed, _ = rc.reference(d, k)
    assert marks
    for p, thr, dist in marks:
        assert bool(zeroed[p + dist]) == (dist == thr + 1) and not zeroed[p]
    rc.run_slices(emu.resolve, [(d, k)], c, seed=len(d))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("stream", ["domino", "edge", "mixture"])
def test_level_seams(stream, c):
    d = {"domino": lambda: rc.domino(3, tiles=6), "edge": lambda: rc.window_edge("tile_seam_late", max_thr=138)[0],
         "mixture": lambda: rc.mixture(0.9, 0.002, n=6 * rc.TILE + 77)}[stream]()
    for cuts in ("seams", "inner_seams"):
        k = rc.CUTS[cuts](len(d))
        sizes = set(np.diff(k).tolist())
        assert cuts != "seams" or {1, 63, 64, 65, 2047, 2048, 2049} <= sizes
        rc.run_slices(emu.resolve, [(d, k)], c, seed=3)


@pytest.mark.parametrize("c", [1, 3])
def test_slices(c):
    slices = rc.slice_batch(small=True)
    assert len(slices) == 5 and len({len(k) for _, k in slices}) == 5
    rc.run_slices(emu.resolve, list(slices), c, seed=2)


@pytest.mark.parametrize("case,cuts", [("zeroed", "one_level"), ("zeroed_no_reset", "one_level"),
                                       ("resets", "early_seams")])
def test_long_lookback(case, cuts):
    d = rc.long_lookback(case)
    k = rc.CUTS[cuts](len(d))
    assert rc.longest_transparent_lookback(d, k, "OC" if case == "resets" else "O") >= 65
    rc.run_slices(emu.resolve, [(d, k)], 1, seed=7)


def test_bad_level_ranges_are_refused():
    off, cut_off = np.array([0, 10], np.int64), np.array([0, 2], np.int32)
    desc, co, sl, err = np.zeros(10, np.uint32), np.ones(10, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    for cuts in ([0, 11], [5, 5], [6, 2], [-1, 4]):
        assert emu.lib().rdoq_emu_resolve(1, off, cut_off, np.array(cuts, np.int32), desc, 1, co, sl, err) == -1


def test_thresholds():
    """the threshold functions with the host's IEEE doubles: the device's division and reciprocal are checked by
    tests/test_gpu_rdoq_edges.py on the same cases"""
    d2, lam, rcf, lim = rc.threshold_inputs()
    out_div, out_recip = emu.thresholds(d2, lam, rcf, lim)
    rc.check_thresholds(d2, lam, rcf, lim, out_div, "division")
    rc.check_thresholds(d2, lam, rcf, lim, out_recip, "reciprocal")
    rc.check_threshold_coverage(d2, lam, lim, out_div)
