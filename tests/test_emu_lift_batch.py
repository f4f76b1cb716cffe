"""The kernels of csrc/lift_batch.hpp -- the lifting transform of a batch of slices over LoD structures the caller
holds -- under the CPU wavefront emulator, through the library's own plan and launch functions
(tests/emu/lift_batch_emu_harness.cpp, guard bytes around every array).  Per slice, forward and inverse equal the C
oracle's lifting over the C oracle's LoD structure (lod_helpers), whatever stands next to the slice.  The check
kernel's verdict is tested here for every kind of bad table, the out-of-range kinds included (no GPU test feeds
those).  Every comparison is exact equality.  No GPU needed."""
import numpy as np
import pytest

import dev_lift_cases as lc


def run_both(name, c, lcp, bitdepth, mode):
    """the batch through the forward and the inverse launch sequence -> (forward, inverse) results of lc.emu_lift"""
    b = lc.batch(name)
    params = b.params(c, lcp, bitdepth, mode)
    xyz = b.xyz if mode == "regions" else None
    fwd = lc.emu_lift(True, params, b.offsets, b.structure(), c, attrs=b.attrs(c, bitdepth), xyz=xyz)
    assert fwd[0] == 0 and fwd[1] == 0, fwd[:3]
    want_lcp = np.stack([e[2] for e in lc.expected(name, c, lcp, bitdepth, mode)])
    inv = lc.emu_lift(False, params, b.offsets, b.structure(), c, coeffs=fwd[4], lcp=want_lcp, xyz=xyz)
    assert inv[0] == 0 and inv[1] == 0, inv[:3]
    return fwd, inv


def check(name, c, lcp, bitdepth, mode):
    b = lc.batch(name)
    exp = lc.expected(name, c, lcp, bitdepth, mode)
    fwd, inv = run_both(name, c, lcp, bitdepth, mode)
    for s in range(len(b.lengths)):
        what = f"{name} c={c} lcp={lcp} {bitdepth} bit {mode}: slice {s} ({b.lengths[s]} points, LoDs {b.npl[s]})"
        np.testing.assert_array_equal(b.slice(fwd[4], s), exp[s][0], err_msg=what + ", coefficients")
        np.testing.assert_array_equal(b.slice(fwd[3], s), exp[s][1], err_msg=what + ", encoder's reconstruction")
        np.testing.assert_array_equal(b.slice(inv[3], s), exp[s][1], err_msg=what + ", decoder's reconstruction")
        if c == 3 and lcp:
            np.testing.assert_array_equal(fwd[5][s], exp[s][2], err_msg=what + ", LCP coefficients")
        else:
            assert (fwd[5][s] == 0x5A).all(), what + ": LCP row written without the flag"
    assert any(e[0].any() for e in exp)
    return fwd, inv


@pytest.mark.parametrize("c,lcp,bitdepth", lc.CONFIGS)
def test_distance_batch_equals_the_oracle_slice_by_slice(c, lcp, bitdepth):
    check("distance", c, lcp, bitdepth, "plain")


@pytest.mark.parametrize("c,lcp,bitdepth", [(3, True, 8), (1, False, 16)])
def test_ragged_batch_equals_the_oracle_slice_by_slice(c, lcp, bitdepth):
    check("ragged", c, lcp, bitdepth, "plain")


@pytest.mark.parametrize("name,c,lcp,bitdepth", [("distance", 3, True, 8), ("distance", 1, False, 16), ("ragged", 3, True, 8)])
def test_regions_on_some_slices_and_none_on_others(name, c, lcp, bitdepth):
    b = lc.batch(name)
    check(name, c, lcp, bitdepth, "regions")
    offs = [b.region_offsets(s, "regions") for s in range(len(b.lengths))]
    assert any(o is None for o in offs) and any(o is not None and o.any() for o in offs)
    # the regions change the result (the table is not idle)
    plain, regions = lc.expected(name, c, lcp, bitdepth), lc.expected(name, c, lcp, bitdepth, "regions")
    assert any((p[0] != r[0]).any() for p, r in zip(plain, regions))


@pytest.mark.parametrize("name,c,lcp,bitdepth", [("distance", 3, True, 8), ("distance", 1, False, 16), ("ragged", 3, False, 8)])
def test_scalable_weights_on_every_other_slice(name, c, lcp, bitdepth):
    check(name, c, lcp, bitdepth, "scalable")
    plain, scalable = lc.expected(name, c, lcp, bitdepth), lc.expected(name, c, lcp, bitdepth, "scalable")
    assert any((p[0] != q[0]).any() for p, q in zip(plain[::2], scalable[::2]))
    for p, q in zip(plain[1::2], scalable[1::2]):
        np.testing.assert_array_equal(p[0], q[0])


def test_the_table_has_its_cases():
    b = lc.batch("distance")
    assert b.lengths == lc.DIST_SIZES
    npl = dict(zip(b.lengths, b.npl))
    assert npl[1] == [1] and npl[2] == [1, 2, 2] and npl[7] == [1, 3, 5, 7, 7] and npl[20] == [1, 4, 10, 15, 20]
    levels = [len(v) for v in b.npl]
    assert [levels[b.lengths.index(n)] for n in (63, 64, 65, 255, 257)] == [5] * 5 and levels[b.lengths.index(4097)] == 10
    assert len(set(levels)) == 4                                                  # differing level counts
    assert any(v[k] == v[k - 1] for v in b.npl for k in range(1, len(v)))         # an empty LoD
    # a step with idle neighbours on both sides of a working slice, forward and inverse (steps 4..8: only the
    # 10-level slice works, between the 5-level slices in front of it and the 20-point slice behind it)
    for inverse in (0, 1):
        works = [[(t + 1 if inverse else len(v) - 1 - t) in range(1, len(v)) and
                  v[t + 1 if inverse else len(v) - 1 - t] > v[(t + 1 if inverse else len(v) - 1 - t) - 1]
                  for v in b.npl] for t in range(max(levels) - 1)]
        assert any(any(not w[s - 1] and w[s] and not w[s + 1] for s in range(1, len(w) - 1)) for w in works)
        assert any(sum(w) == 1 for w in works)                                    # a step in which one slice works
    r = lc.batch("ragged")
    assert len(r.lengths) == 300 and min(r.lengths) == 1 and max(r.lengths) == 40
    assert len({len(v) for v in r.npl}) > 1


def test_the_launches_follow_the_levels_not_the_slices():
    """forward at most 7 + 7 (L - 1) launches, inverse at most 5 + 4 (L - 1), L the batch's largest num_lods"""
    for name in ("distance", "ragged"):
        b = lc.batch(name)
        L = max(len(v) for v in b.npl)
        fwd, inv = run_both(name, 3, True, 8, "scalable")
        assert fwd[2] <= 7 + 7 * (L - 1) and inv[2] <= 5 + 4 * (L - 1), (name, L, fwd[2], inv[2])
        fwd, inv = run_both(name, 1, False, 8, "plain")
        assert fwd[2] <= 4 + 7 * (L - 1) and inv[2] <= 4 + 4 * (L - 1), (name, L, fwd[2], inv[2])
    d, r = lc.batch("distance"), lc.batch("ragged")
    assert len(r.lengths) == 30 * len(d.lengths)


BAD_TABLES = ("count of 4", "point index of n_s", "negative neighbour", "neighbour in the predictor's own level",
              "neighbour at n_s")


@pytest.mark.parametrize("forward", [True, False])
@pytest.mark.parametrize("kind", BAD_TABLES)
def test_the_check_kernel_refuses_and_nothing_is_touched(kind, forward):
    b = lc.batch("distance")
    c, lcp, bitdepth = 3, True, 8
    nc, ni, nw, ix = (a.copy() for a in b.structure())
    s = b.lengths.index(65)           # a slice in the middle of the batch
    base, n, npl = int(b.offsets[s]), b.lengths[s], b.npl[s]
    i = npl[2] + 1                    # a predictor of level 3 with a neighbour
    assert nc[base + i] >= 1 and npl[2] < i < npl[3]
    if kind == "count of 4":
        nc[base + i] = 4
    elif kind == "point index of n_s":
        ix[base + i] = n
    elif kind == "negative neighbour":
        ni[base + i, 0] = -1
    elif kind == "neighbour in the predictor's own level":
        ni[base + i, 0] = npl[2]
    else:
        ni[base + i, 0] = n
    params = b.params(c, lcp, bitdepth)
    attrs = b.attrs(c, bitdepth) if forward else None
    coeffs = None if forward else np.concatenate([e[0] for e in lc.expected("distance", c, lcp, bitdepth)])
    rcode, verdict, launches, a, co, l = lc.emu_lift(forward, params, b.offsets, (nc, ni, nw, ix), c, attrs=attrs, coeffs=coeffs)
    # (the harness has compared every output and working array and all guard bands with what they were)
    assert rcode == 0 and verdict != 0, (rcode, verdict)
    if forward:
        np.testing.assert_array_equal(a, attrs)
        assert (co == lc.PATTERN).all()
    else:
        assert (a == lc.PATTERN).all()
        np.testing.assert_array_equal(co, coeffs)
    assert (l == 0x5A).all()
    # the same tables unspoilt pass
    assert lc.emu_lift(forward, params, b.offsets, b.structure(), c, attrs=attrs, coeffs=coeffs)[1] == 0
