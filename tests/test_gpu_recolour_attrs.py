"""GPU parity of gpcc_recolour_attrs: every attribute of a call identical to what pcc::recolour gives for it alone
(the compiled reference where present, else the oracle restatement) and to Context.recolour, ties included --
whatever stands next to it in the call, at every size around a workgroup and a wavefront, under the finite forward
geometry limits, and from one call to the next (the atomics fill the backward lists in any order)."""
import numpy as np
import pytest

import recolour_attrs_cases as rac
from mpeg_pcc_tmc13_amd import recolour_params, synth
from test_emu_recolour import requantise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    assert hasattr(c, "recolour_attrs")
    yield c
    c.close()


def with_depth(p, bitdepth):
    q = type(p).from_buffer_copy(p)
    q.bitdepth = bitdepth
    return q


def run(ctx):
    return lambda p, xyz, attrs, tgt, scale: ctx.recolour_attrs(p, xyz, attrs, tgt, scale=scale)


@pytest.mark.parametrize("kind,scale,kw", rac.MATRIX)
def test_each_attribute_gets_its_own_result_in_any_company(ctx, kind, scale, kw):
    """two attributes, the two reversed, and four (colour, reflectance, colour + 9 mod 256, reflectance reversed)"""
    rac.check_orders(run(ctx), kind, scale, kw, rac.TWO + rac.REVERSED_AND_FOUR)


@pytest.mark.parametrize("kind,scale,kw", [rac.MATRIX[0], rac.MATRIX[4], rac.MATRIX[6], rac.MATRIX[11]])
def test_equals_recolour_per_attribute_and_alone(ctx, kind, scale, kw):
    p, xyz, attrs, tgt, want = rac.case(kind, scale, rac.key(kw))
    got = ctx.recolour_attrs(p, xyz, attrs[:2], tgt, scale=scale)
    for (a, d), g in zip(attrs[:2], got):
        single = ctx.recolour(with_depth(p, d), xyz, a, tgt, scale=scale)
        np.testing.assert_array_equal(g, single)
        # a call with one attribute is gpcc_recolour
        np.testing.assert_array_equal(ctx.recolour_attrs(p, xyz, [(a, d)], tgt, scale=scale)[0], single)


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 255, 256, 257])
def test_target_counts_around_a_wavefront_and_a_workgroup(ctx, nt):
    """the first rows of the requantised cloud (1 500 source points: with one target its backward list holds them all,
    and a lane's work on a list grows with the square of its length)"""
    xyz, pair = rac.cloud("dense", 6000)
    xyz = np.ascontiguousarray(xyz[:1500])
    pair = [(np.ascontiguousarray(a[:1500]), d) for a, d in pair]
    p = recolour_params(bitdepth=8)
    tgt = requantise(xyz, 0.5)
    assert len(tgt) >= 257
    tgt = np.ascontiguousarray(tgt[:nt])
    got = ctx.recolour_attrs(p, xyz, pair, tgt, scale=0.5)
    for (a, d), g in zip(pair, got):
        np.testing.assert_array_equal(g, rac.alone(p, xyz, a, d, tgt, scale=0.5))


@pytest.mark.parametrize("ns", [255, 256, 257])
def test_source_counts_around_a_workgroup(ctx, ns):
    xyz, pair = rac.cloud("dense", 6000)
    xyz = np.ascontiguousarray(xyz[:ns])
    pair = [(np.ascontiguousarray(a[:ns]), d) for a, d in pair]
    p = recolour_params(bitdepth=8, max_attr_bwd=300.0)
    tgt = requantise(xyz, 0.5)
    got = ctx.recolour_attrs(p, xyz, pair, tgt, scale=0.5)
    for (a, d), g in zip(pair, got):
        np.testing.assert_array_equal(g, rac.alone(p, xyz, a, d, tgt, scale=0.5))


@pytest.mark.parametrize("kind,scale,kw", rac.GEOMETRY_LIMITS)
def test_finite_forward_geometry_limit(ctx, kind, scale, kw):
    rac.check_orders(run(ctx), kind, scale, kw, rac.TWO)


def test_two_calls_give_identical_outputs(ctx):
    p, xyz, attrs, tgt, want = rac.case("dense", 0.125, rac.key(dict(k_bwd=4, max_attr_bwd=400.0)))
    first = ctx.recolour_attrs(p, xyz, attrs, tgt, scale=0.125)
    second = ctx.recolour_attrs(p, xyz, attrs, tgt, scale=0.125)
    for f, s, w in zip(first, second, want):
        np.testing.assert_array_equal(f, s)
        np.testing.assert_array_equal(f, w)


def test_duplicates_offset_and_small_clouds(ctx):
    xyz, a = synth.dense_cloud(3000, seed=5, bits=6)
    xyz = np.concatenate([xyz, xyz[::3], xyz[::7]])
    a = np.concatenate([a, (a[::3] + 9) % 256, (a[::7] + 31) % 256]).astype(np.int32)
    b = np.random.default_rng(77).integers(0, 1024, (len(xyz), 1)).astype(np.int32)
    p = recolour_params(bitdepth=8)
    for scale, off in ((1.0, (0, 0, 0)), (0.5, (3, -2, 5))):
        tgt = np.unique(np.rint(xyz.astype(np.float64) * scale).astype(np.int32) - np.array(off, dtype=np.int32), axis=0)
        got = ctx.recolour_attrs(p, xyz, [(a, 8), (b, 10)], tgt, scale=scale, offset=off)
        np.testing.assert_array_equal(got[0], rac.alone(p, xyz, a, 8, tgt, scale=scale, offset=off))
        np.testing.assert_array_equal(got[1], rac.alone(p, xyz, b, 10, tgt, scale=scale, offset=off))
    xyz, a = synth.random_cloud(8, seed=2, bits=3, c=3)
    b = np.random.default_rng(77).integers(0, 1024, (8, 1)).astype(np.int32)
    for tgt in (xyz, xyz[:1]):
        got = ctx.recolour_attrs(p, xyz, [(b, 10), (a, 8)], tgt)
        np.testing.assert_array_equal(got[0], rac.alone(p, xyz, b, 10, tgt))
        np.testing.assert_array_equal(got[1], rac.alone(p, xyz, a, 8, tgt))


@pytest.mark.parametrize("kind,scale", [("dense", 0.5), ("lidar", 0.25)])
def test_twenty_thousand_points(ctx, kind, scale):
    """several levels of the tree build above the subtrees; both attribute limits"""
    rac.check_orders(run(ctx), kind, scale, dict(max_attr_fwd=200.0, max_attr_bwd=300.0), rac.TWO, n=20000)
