"""The slice-level inter / intra decision on the MI355X: gpcc_lift_encode_attr_rdo / gpcc_pred_encode_attr_rdo run both
candidates of every fixture case (tests/golden/slice_rdo_golden.npz, the compiled reference's AttributeEncoder::encode
with attrInterIntraSliceRDO) in one call.  Both candidates equal what the single-candidate entries give, the distortion
sums equal the reference's, the byte counts (the device's binary decisions on the reference's arithmetic coder) and with
them the decision equal the reference's, and the winner decodes to its reconstruction."""
import numpy as np
import pytest

import lod_helpers as lh
import slice_rdo_cases as sc

pytestmark = pytest.mark.gpu
GPCC_ERR_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


def both(ctx, inp):
    """the new entry -> (values [2,n], recon [2,n], dist [2])"""
    n = len(inp["xyz"])
    fn = ctx.lift_encode_attr_rdo if inp["transform"] == 2 else ctx.pred_encode_attr_rdo
    return fn(inp["lod_inter"], inp["lod_intra"], sc.transform_params(inp, [n]), inp["xyz"], inp["attrs"], inp["xyz_ref"],
              inp["attrs_ref"], inp["search_range"], inp["frame_distance"])


def separately(ctx, inp):
    """the existing single-candidate entries -> [(values [n,1], recon [n,1], structure or None)] inter, intra"""
    xyz, attrs = inp["xyz"], inp["attrs"]
    lod = ctx.lod_build_inter(inp["lod_inter"], xyz, inp["xyz_ref"], inp["search_range"], inp["frame_distance"])
    p = sc.transform_params(inp, lod["npl"])
    if inp["transform"] == 2:
        v0, r0 = ctx.lift_inter(True, p, lod, inp["attrs_ref"], attrs=attrs)
        v1, r1, _, _ = ctx.lift_encode_attr(inp["lod_intra"], sc.transform_params(inp, [len(xyz)]), xyz, attrs)
    else:
        v0, r0 = ctx.pred_inter(True, p, lod, inp["attrs_ref"], attrs=attrs)
        v1, r1, _, _ = ctx.pred_encode_attr(inp["lod_intra"], sc.transform_params(inp, [len(xyz)]), xyz, attrs)
    return [(v0, r0, lod), (v1, r1, None)]


def coded_bytes(ctx, values, n):
    runs, vals, trailing = ctx.zero_run_pack(values, n, 1, 0)
    bins = ctx.binarise_symbols(runs, vals, trailing, 1)
    return len(lh.ref_entropy_encode_bins(bins, n))


@pytest.mark.parametrize("name", sc.NAMES)
def test_both_candidates_vs_the_separate_entries_and_the_reference(ctx, name):
    inp, c = sc.inputs(name), sc.case(name)
    src = inp["attrs"].copy()
    values, recon, dist = both(ctx, inp)
    np.testing.assert_array_equal(inp["attrs"], src, err_msg="the caller's attributes were written")
    for k, (v, r, _) in enumerate(separately(ctx, inp)):
        np.testing.assert_array_equal(values[k], v[:, 0], err_msg=f"values of candidate {k}")
        np.testing.assert_array_equal(recon[k], r[:, 0], err_msg=f"reconstruction of candidate {k}")
    np.testing.assert_array_equal(dist, c["dist"])
    np.testing.assert_array_equal(dist, np.abs(recon.astype(np.int64) - src[:, 0]).sum(axis=1))
    # the reference's reconstruction is the winner's
    assert sc.digest(recon[int(c["intra_wins"])]) == c["recon_sha"]


@pytest.mark.parametrize("name", sc.NAMES)
def test_byte_counts_and_decision_vs_the_reference(ctx, name):
    if not lh.entropy_available():
        pytest.skip("oracle/_ref/libtmc3_entropy.so not built")
    from mpeg_pcc_tmc13_amd.raht import slice_rdo_choose
    inp, c = sc.inputs(name), sc.case(name)
    n = len(inp["xyz"])
    values, recon, dist = both(ctx, inp)
    nbytes = [coded_bytes(ctx, values[k], n) for k in (0, 1)]
    assert nbytes == c["bytes"].tolist()
    win, cost = slice_rdo_choose(dist[0], nbytes[0], dist[1], nbytes[1], inp["init_qp_minus4"])
    assert win == c["intra_wins"]
    np.testing.assert_array_equal(np.array(cost), sc.golden()[name + "/cost"])


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_winner_decodes_to_its_reconstruction(ctx, name):
    inp, c = sc.inputs(name), sc.case(name)
    xyz = inp["xyz"]
    values, recon, _ = both(ctx, inp)
    k = int(c["intra_wins"])
    v = values[k].reshape(-1, 1)
    if k == 0:
        lod = ctx.lod_build_inter(inp["lod_inter"], xyz, inp["xyz_ref"], inp["search_range"], inp["frame_distance"])
        p = sc.transform_params(inp, lod["npl"])
        inv = ctx.lift_inter if inp["transform"] == 2 else ctx.pred_inter
        kw = dict(coeffs=v) if inp["transform"] == 2 else dict(values=v)
        dec = inv(False, p, lod, inp["attrs_ref"], **kw)[1]
    elif inp["transform"] == 2:
        dec = ctx.lift_decode_attr(inp["lod_intra"], sc.transform_params(inp, [len(xyz)]), xyz, v)
    else:
        dec = ctx.pred_decode_attr(inp["lod_intra"], sc.transform_params(inp, [len(xyz)]), xyz, v)
    np.testing.assert_array_equal(dec[:, 0], recon[k])


@pytest.mark.parametrize("transform", [2, 1])
def test_a_declined_call_leaves_the_slice_intact(ctx, transform):
    from mpeg_pcc_tmc13_amd import _lib
    inp = sc.inputs("lift_tiny" if transform == 2 else "pred_tiny")
    src = inp["attrs"].copy()
    before = ctx.stats()
    inp["lod_inter"].canonical_point_order_flag = 1
    with pytest.raises(_lib.GpccError) as e:
        both(ctx, inp)
    assert e.value.code == GPCC_ERR_UNSUPPORTED
    np.testing.assert_array_equal(inp["attrs"], src)
    after = ctx.stats()
    assert after["calls_unsupported"] == before["calls_unsupported"] + 1
    # ... and the context goes on working
    inp["lod_inter"].canonical_point_order_flag = 0
    _, _, dist = both(ctx, inp)
    np.testing.assert_array_equal(dist, sc.case(inp["name"])["dist"])


def test_one_million_points_self_consistent(ctx):
    """a lidar-like slice of 1 M points: the one call against the separate entries, the sums against numpy"""
    from mpeg_pcc_tmc13_amd import synth
    xyz, a = synth.lidar_cloud(1000000, seed=71, refl_noise=24)
    attrs = np.ascontiguousarray(a[:, :1], dtype=np.int32)
    rng = np.random.default_rng(72)
    keep = rng.random(len(xyz)) > 0.1
    xr = np.clip(xyz + rng.integers(-1, 2, size=xyz.shape), 0, None)[keep].astype(np.int32)
    ar = np.clip(attrs + rng.integers(-5, 6, size=attrs.shape), 0, 255)[keep].astype(np.int32)
    inp = dict(sc.inputs("lift_tiny"), xyz=xyz, attrs=attrs, xyz_ref=xr, attrs_ref=ar, layers=[28], init_qp_minus4=24)
    src = attrs.copy()
    values, recon, dist = both(ctx, inp)
    np.testing.assert_array_equal(attrs, src)
    for k, (v, r, _) in enumerate(separately(ctx, inp)):
        np.testing.assert_array_equal(values[k], v[:, 0], err_msg=f"values of candidate {k}")
        np.testing.assert_array_equal(recon[k], r[:, 0], err_msg=f"reconstruction of candidate {k}")
    np.testing.assert_array_equal(dist, np.abs(recon.astype(np.int64) - src[:, 0]).sum(axis=1))
    assert dist[0] > 0 and dist[1] > 0
