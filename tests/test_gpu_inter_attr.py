"""LoD slices with attribute inter prediction on the MI355X.

The reference-frame crop (gpcc_dev_attr_ref_crop / gpcc_attr_ref_crop) against every case of
tests/golden/ref_crop_golden.npz, i.e. against the compiled reference's computeBoundingBox + Box3::contains loop:
offsets, boxes, arrays or digests, the capacity rule and the domain's error word.

The one-call entries (gpcc_{lift,pred}_{encode,decode}_attr_inter) against the existing two-call path, the CPU oracle
chain of lod_helpers and -- where inter wins the slice-level decision -- the compiled reference's reconstruction
(tests/golden/slice_rdo_golden.npz).

The device tier (gpcc_dev_*_attr_inter) on batches against the oracle, and the chain frame t (intra, device) ->
crop -> frame t + 1 (inter, device) with nothing but the offsets passing through the host.  Bit-exact, no tolerance."""
import numpy as np
import pytest

import inter_attr_cases as ic
import lod_helpers as lh
import oracle_loader as ol
import ref_crop_cases as rc
import slice_rdo_cases as sc

pytestmark = pytest.mark.gpu
GPCC_ERR_INVALID_ARG, GPCC_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


def to_dev(a, lead=0):
    """a flat int32 device tensor holding `a` behind `lead` spare words -> (tensor, address of the data)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    t = torch.zeros(len(a) + lead, dtype=torch.int32, device="cuda:0")
    t[lead:] = torch.from_numpy(a).to("cuda:0")
    return t, t.data_ptr() + 4 * lead


def filled(words, value=-7):
    import torch
    return torch.full((max(int(words), 1),), value, dtype=torch.int32, device="cuda:0")


# ---- the crop -------------------------------------------------------------------------------------------------
def dev_crop(ctx, c, capacity=None):
    """the whole batch in one device call -> (ref_offsets, bbox, positions, attributes, the output tensors).
    An unaligned case: the frame's arrays start one point behind torch's allocation."""
    import torch
    fa = c["frame_attrs"]
    nf, ca = fa.shape
    lead = 1 if c["unaligned"] else 0
    t_xyz, p_xyz = to_dev(c["xyz"])
    t_fx, p_fx = to_dev(c["frame_xyz"], 3 * lead)
    t_fa, p_fa = to_dev(fa, ca * lead)
    cap = (len(c["offsets"]) - 1) * nf if capacity is None else capacity
    t_ox, t_oa = filled(3 * cap), filled(ca * cap)
    torch.cuda.synchronize()
    try:
        ro, bbox = ctx.dev_attr_ref_crop(c["offsets"], p_xyz, nf, p_fx, p_fa, ca, t_ox.data_ptr(), t_oa.data_ptr(), cap,
                                         want_bbox=True)
    finally:
        torch.cuda.synchronize()  # (the tensors above are idle again, also behind a call that failed)
    k = int(ro[-1])
    return ro, bbox, t_ox.cpu().numpy()[:3 * k].reshape(-1, 3), t_oa.cpu().numpy()[:ca * k].reshape(-1, ca), (t_ox, t_oa)


def host_crop(ctx, c):
    """one host call per slice of the case"""
    off = c["offsets"]
    boxes, ox, oa, ro = [], [], [], [0]
    for s in range(len(off) - 1):
        x, a, b = ctx.attr_ref_crop(c["xyz"][off[s]:off[s + 1]], c["frame_xyz"], c["frame_attrs"])
        boxes.append(b.reshape(6))
        ox.append(x)
        oa.append(a)
        ro.append(ro[-1] + len(x))
    return np.array(ro, np.int64), np.stack(boxes), np.concatenate(ox), np.concatenate(oa)


@pytest.mark.parametrize("name", rc.NAMES)
def test_crop_matches_the_reference_in_both_tiers(name, ctx):
    c = rc.case(name)
    ro, bbox, ox, oa, _ = dev_crop(ctx, c)
    rc.check(c, bbox, ro, ox, oa)
    ro, bbox, ox, oa = host_crop(ctx, c)
    rc.check(c, bbox, ro, ox, oa)


@pytest.mark.parametrize("name", ["alternating_1025_c1", "lidar8", "ragged300"])
def test_crop_capacity(name, ctx):
    """exactly enough is enough; one point less: GPCC_ERR_INVALID_ARG, the offsets filled, nothing written -- and a
    call with capacity 0 and no output buffers sizes them"""
    from mpeg_pcc_tmc13_amd._lib import GpccError
    c = rc.case(name)
    total = int(c["ref_offsets"][-1])
    ro, bbox, ox, oa, _ = dev_crop(ctx, c, capacity=total)
    rc.check(c, bbox, ro, ox, oa)
    import torch
    ca = c["frame_attrs"].shape[1]
    t_xyz, p_xyz = to_dev(c["xyz"])
    t_fx, p_fx = to_dev(c["frame_xyz"])
    t_fa, p_fa = to_dev(c["frame_attrs"])
    t_ox, t_oa = filled(3 * total), filled(ca * total)
    torch.cuda.synchronize()
    for cap, ox_ptr, oa_ptr in ((total - 1, t_ox.data_ptr(), t_oa.data_ptr()), (0, None, None)):
        with pytest.raises(GpccError) as e:
            ctx.dev_attr_ref_crop(c["offsets"], p_xyz, len(c["frame_xyz"]), p_fx, p_fa, ca, ox_ptr, oa_ptr, cap)
        assert e.value.code == GPCC_ERR_INVALID_ARG and "capacity" in str(e.value)
        np.testing.assert_array_equal(e.value.ref_offsets, c["ref_offsets"])
        ctx.synchronize()
        assert bool((t_ox == -7).all()) and bool((t_oa == -7).all())
    if len(c["offsets"]) == 2:
        with pytest.raises(GpccError) as e:
            ctx.attr_ref_crop(c["xyz"], c["frame_xyz"], c["frame_attrs"], capacity=total - 1)
        assert e.value.code == GPCC_ERR_INVALID_ARG
        x, a, b = ctx.attr_ref_crop(c["xyz"], c["frame_xyz"], c["frame_attrs"], capacity=total)
        rc.check(c, b, c["ref_offsets"], x, a)


def test_crop_coordinate_outside_the_domain_is_an_error_code(ctx):
    from mpeg_pcc_tmc13_amd._lib import GpccError
    c = rc.case("alternating_1025_c1")
    for where in ("frame", "slice"):
        bad = dict(c, frame_xyz=c["frame_xyz"].copy(), xyz=c["xyz"].copy())
        if where == "frame":
            bad["frame_xyz"][1030 % len(bad["frame_xyz"])] = (5, 1 << 21, 5)
        else:
            bad["xyz"][1] = (150, 150, 1 << 21)
        with pytest.raises(GpccError) as e:
            dev_crop(ctx, bad)
        assert e.value.code == GPCC_ERR_INVALID_ARG and "2^21" in str(e.value), where
        ctx.synchronize()  # (reported once)
        with pytest.raises(GpccError) as e:
            ctx.attr_ref_crop(bad["xyz"], bad["frame_xyz"], bad["frame_attrs"])
        assert e.value.code == GPCC_ERR_INVALID_ARG
    # the context is as good as before
    ro, bbox, ox, oa, _ = dev_crop(ctx, c)
    rc.check(c, bbox, ro, ox, oa)


# ---- one call per slice ---------------------------------------------------------------------------------------
def one_call(ctx, inp, encode, values=None):
    n = len(inp["xyz"])
    p = sc.transform_params(inp, [n])
    v, r, idx = ctx.attr_inter(inp["transform"] == 1, encode, inp["lod_inter"], p, inp["xyz"], inp["xyz_ref"],
                               inp["attrs_ref"], inp["search_range"], inp["frame_distance"], attrs=inp["attrs"],
                               values=values)
    return v, r, idx, list(p.num_points_in_lod[:p.num_lods])


def two_calls(ctx, inp):
    lod = ctx.lod_build_inter(inp["lod_inter"], inp["xyz"], inp["xyz_ref"], inp["search_range"], inp["frame_distance"])
    p = sc.transform_params(inp, lod["npl"])
    fn = ctx.lift_inter if inp["transform"] == 2 else ctx.pred_inter
    v, r = fn(True, p, lod, inp["attrs_ref"], attrs=inp["attrs"])
    return v, r, lod


def oracle_chain(inp):
    st = lh.oracle_lod_generate_inter(inp["xyz"], inp["xyz_ref"], inp["lod_inter"], inp["search_range"],
                                      inp["frame_distance"])
    p = sc.transform_params(inp, st["npl"])
    if inp["transform"] == 2:
        v, r = lh.lift_inter(ol.oracle(), True, p, st, inp["attrs"], inp["attrs_ref"])
    else:
        v, r, _ = lh.pred_inter(True, p, st, inp["attrs_ref"], attrs=inp["attrs"])
    used = np.arange(3)[None, :] < st["nc"][:, None]
    return v, r, st, int((st["ref"].astype(bool) & used).sum())


@pytest.mark.parametrize("name", sc.NAMES)
def test_one_call_vs_two_calls_the_oracle_and_the_reference(ctx, name):
    inp, c = sc.inputs(name), sc.case(name)
    v, r, idx, npl = one_call(ctx, inp, True)
    # the existing two-call path
    v2, r2, lod = two_calls(ctx, inp)
    np.testing.assert_array_equal(v, v2, err_msg="values vs the two-call path")
    np.testing.assert_array_equal(r, r2, err_msg="reconstruction vs the two-call path")
    np.testing.assert_array_equal(idx, lod["indexes"])
    assert npl == list(lod["npl"])
    # the CPU oracle chain
    ov, orec, st, flagged = oracle_chain(inp)
    assert flagged > 0, "no neighbour lives in the reference frame: the case shows nothing"
    np.testing.assert_array_equal(v, ov, err_msg="values vs the oracle")
    np.testing.assert_array_equal(r, orec, err_msg="reconstruction vs the oracle")
    np.testing.assert_array_equal(idx, st["indexes"])
    # the compiled reference's encoder, where it kept the inter candidate
    if not c["intra_wins"]:
        assert sc.digest(r[:, 0]) == c["recon_sha"]
    # the decoder gives the encoder's reconstruction
    _, dec, didx, dnpl = one_call(ctx, inp, False, values=v)
    np.testing.assert_array_equal(dec, r)
    np.testing.assert_array_equal(didx, idx)
    assert dnpl == npl


def test_the_reference_keeps_the_inter_candidate_in_cases_of_both_transforms():
    kept = [n for n in sc.NAMES if not sc.case(n)["intra_wins"]]
    assert any(n.startswith("lift_") for n in kept) and any(n.startswith("pred_") for n in kept)


@pytest.mark.parametrize("transform", [2, 1])
@pytest.mark.parametrize("encode", [True, False])
def test_a_declined_call_leaves_the_slice_intact(ctx, transform, encode):
    """the entry gets the caller's own arrays (in_place), as a C caller's: what it reads and what it would have written"""
    from mpeg_pcc_tmc13_amd import _lib
    inp = sc.inputs("lift_tiny" if transform == 2 else "pred_tiny")
    n = len(inp["xyz"])
    good_v, good_r, _, _ = one_call(ctx, inp, True)
    # encoder: attrs in (the source), values out; decoder: values in, attrs out
    attrs = np.ascontiguousarray(inp["attrs"], np.int32).copy() if encode else np.full((n, 1), -7, np.int32)
    values = np.full((n, 1), -7, np.int32) if encode else good_v.copy()
    attrs_before, values_before = attrs.copy(), values.copy()
    p = sc.transform_params(inp, [n])
    before = ctx.stats()
    inp["lod_inter"].canonical_point_order_flag = 1
    with pytest.raises(_lib.GpccError) as e:
        ctx.attr_inter(transform == 1, encode, inp["lod_inter"], p, inp["xyz"], inp["xyz_ref"], inp["attrs_ref"],
                       inp["search_range"], inp["frame_distance"], attrs=attrs, values=values, in_place=True)
    assert e.value.code == GPCC_ERR_UNSUPPORTED
    np.testing.assert_array_equal(attrs, attrs_before)
    np.testing.assert_array_equal(values, values_before)
    assert list(p.num_points_in_lod[:p.num_lods]) == [n]
    after = ctx.stats()
    assert after["calls_unsupported"] == before["calls_unsupported"] + 1
    assert after["calls_ok"] == before["calls_ok"] and after["calls_failed"] == before["calls_failed"]
    # ... and the context goes on working, on the same arrays
    inp["lod_inter"].canonical_point_order_flag = 0
    ctx.attr_inter(transform == 1, encode, inp["lod_inter"], p, inp["xyz"], inp["xyz_ref"], inp["attrs_ref"],
                   inp["search_range"], inp["frame_distance"], attrs=attrs, values=values, in_place=True)
    np.testing.assert_array_equal(values, good_v)
    np.testing.assert_array_equal(attrs, good_r)


# ---- the device tier ------------------------------------------------------------------------------------------
def dev_batch(ctx, predicting, encode, batch, st, values=None):
    """a batch of (xyz, attrs, xyz_ref, attrs_ref) slices through the device-tier entry -> per slice
    (values, recon, indexes, npl)"""
    import torch
    off = np.concatenate([[0], np.cumsum([len(b[0]) for b in batch])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum([len(b[2]) for b in batch])]).astype(np.int64)
    t_xyz, p_xyz = to_dev(np.concatenate([b[0] for b in batch]))
    t_a, p_a = to_dev(np.concatenate([b[1] for b in batch]) if encode else np.zeros(off[-1], np.int32))
    t_v, p_v = to_dev(np.zeros(off[-1], np.int32) if encode else np.concatenate(values))
    t_xr, p_xr = to_dev(np.concatenate([b[2] for b in batch]))
    t_ar, p_ar = to_dev(np.concatenate([b[3] for b in batch]))
    t_ix = filled(off[-1])
    lp = ic.lod(predicting)
    plist = [ic.params(predicting, lp, [len(b[0])], st["qp"], st["direct"]) for b in batch]
    torch.cuda.synchronize()
    ctx.dev_attr_inter(predicting, encode, lp, plist, off, p_xyz, p_a, p_v, ro, p_xr, p_ar, st["search_range"],
                       st["frame_distance"], d_indexes=t_ix.data_ptr())
    ctx.synchronize()
    a, v, ix = t_a.cpu().numpy(), t_v.cpu().numpy(), t_ix.cpu().numpy()
    return [(v[off[s]:off[s + 1]].reshape(-1, 1), a[off[s]:off[s + 1]].reshape(-1, 1), ix[off[s]:off[s + 1]],
             list(plist[s].num_points_in_lod[:plist[s].num_lods])) for s in range(len(batch))]


def check_batch(ctx, predicting, batch, st):
    want = [ic.oracle(predicting, *b, st["search_range"], st["frame_distance"], st["qp"], st["direct"]) for b in batch]
    assert all(w["flagged"] > 0 for w in want), "a slice without a neighbour in its frame shows nothing"
    got = dev_batch(ctx, predicting, True, batch, st)
    for s, (g, w) in enumerate(zip(got, want)):
        shape = (len(batch[s][0]), len(batch[s][2]))
        np.testing.assert_array_equal(g[0], w["values"], err_msg=f"values of slice {s} {shape}")
        np.testing.assert_array_equal(g[1], w["recon"], err_msg=f"reconstruction of slice {s} {shape}")
        np.testing.assert_array_equal(g[2], w["indexes"], err_msg=f"indexes of slice {s} {shape}")
        assert g[3] == list(w["npl"]), (s, shape)
    dec = dev_batch(ctx, predicting, False, batch, st, values=[w["values"].reshape(-1) for w in want])
    for s, (d, w) in enumerate(zip(dec, want)):
        np.testing.assert_array_equal(d[1], w["recon"], err_msg=f"decoder, slice {s}")


@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("predicting", [False, True])
def test_device_tier_batch_vs_the_oracle(ctx, predicting, setting):
    """n in {1, 2, 65, 1 025} against frames of {1, 64, 1 500} points in one batch"""
    check_batch(ctx, predicting, ic.grid_batch(), ic.SETTINGS[setting])


@pytest.mark.parametrize("predicting", [False, True])
def test_device_tier_ragged_batch_on_all_lanes(ctx, predicting):
    batch = ic.ragged_batch()
    assert len(batch) == 40
    check_batch(ctx, predicting, batch, ic.SETTINGS["fd1_sr128"])


@pytest.mark.parametrize("predicting", [False, True])
def test_chain_frame_to_frame_stays_in_hbm(ctx, predicting):
    """frame t through the intra device entry; its positions and its reconstruction, where the coder left it, through
    the crop for the four slices of frame t + 1; those through the inter device entries.  Only ref_offsets pass
    through the host between the calls; the copies to the host below are the test's comparison."""
    import torch
    from mpeg_pcc_tmc13_amd import synth
    st = ic.SETTINGS["fd1_sr128"]
    xt, at = synth.lidar_cloud(6000, seed=31, refl_noise=24)
    rng = np.random.default_rng(33)
    x1 = np.clip(xt + rng.integers(-2, 3, xt.shape), 0, (1 << 18) - 1).astype(np.int32)
    a1 = np.clip(at + rng.integers(-6, 7, at.shape), 0, 255).astype(np.int32)
    nt, slices = len(xt), 4
    off1 = np.linspace(0, len(x1), slices + 1).astype(np.int64)
    lp = ic.lod(predicting)
    # every buffer of the chain up front, and torch's stream idle before the first call: the context's stream does not
    # order against it
    t_xt, p_xt = to_dev(xt)
    t_at, p_at = to_dev(at)
    t_vt = filled(nt, 0)
    t_x1, p_x1 = to_dev(x1)
    t_xr, t_ar = filled(3 * slices * nt), filled(slices * nt)
    t_a1, p_a1 = to_dev(a1)
    t_v1, t_dec = filled(len(x1), 0), filled(len(x1), 0)
    sizes1 = [int(off1[s + 1] - off1[s]) for s in range(slices)]
    pt = [ic.params(predicting, lp, [nt], st["qp"], st["direct"])]
    p1 = [ic.params(predicting, lp, [m], st["qp"], st["direct"]) for m in sizes1]
    p1d = [ic.params(predicting, lp, [m], st["qp"], st["direct"]) for m in sizes1]
    torch.cuda.synchronize()
    # frame t, intra
    (ctx.dev_pred_attr if predicting else ctx.dev_lift_attr)(True, lp, pt, [0, nt], p_xt, p_at, t_vt.data_ptr(), 1)
    # the crop: t_at now holds the reconstruction of frame t
    ro = ctx.dev_attr_ref_crop(off1, p_x1, nt, p_xt, p_at, 1, t_xr.data_ptr(), t_ar.data_ptr(), slices * nt)
    # frame t + 1, inter: encoder, then the decoder over its values
    ctx.dev_attr_inter(predicting, True, lp, p1, off1, p_x1, p_a1, t_v1.data_ptr(), ro, t_xr.data_ptr(), t_ar.data_ptr(),
                       st["search_range"], st["frame_distance"])
    ctx.dev_attr_inter(predicting, False, lp, p1d, off1, p_x1, t_dec.data_ptr(), t_v1.data_ptr(), ro, t_xr.data_ptr(),
                       t_ar.data_ptr(), st["search_range"], st["frame_distance"])
    ctx.synchronize()
    # the oracle over the numpy-cropped frame
    recon_t = t_at.cpu().numpy().reshape(-1, 1)
    assert not np.array_equal(recon_t, at), "frame t was coded losslessly: the chain would show less"
    bbox, want_ro, ox, oa = rc.crop_numpy(x1, off1, xt, recon_t)
    np.testing.assert_array_equal(ro, want_ro)
    kept = np.diff(want_ro)
    assert (kept > 0).all() and (kept < nt).any()
    v1, r1, dec = t_v1.cpu().numpy(), t_a1.cpu().numpy(), t_dec.cpu().numpy()
    for s in range(slices):
        lo, hi = off1[s], off1[s + 1]
        w = ic.oracle(predicting, x1[lo:hi], a1[lo:hi], ox[want_ro[s]:want_ro[s + 1]], oa[want_ro[s]:want_ro[s + 1]],
                      st["search_range"], st["frame_distance"], st["qp"], st["direct"])
        assert w["flagged"] > 0
        np.testing.assert_array_equal(v1[lo:hi], w["values"][:, 0], err_msg=f"values of slice {s}")
        np.testing.assert_array_equal(r1[lo:hi], w["recon"][:, 0], err_msg=f"reconstruction of slice {s}")
        np.testing.assert_array_equal(dec[lo:hi], w["recon"][:, 0], err_msg=f"decoder, slice {s}")


def test_device_tier_frame_beyond_one_capped_grid(ctx):
    """the library caps its grids at 2 048 workgroups of 256 threads: a frame of more than 524 288 points (its staging
    for the lifting coder) and of more than 174 762 points (the range check over its coordinates) takes the grid-stride
    turns of the two kernels.  The slice sits where the frame's LAST points are."""
    from mpeg_pcc_tmc13_amd import synth
    from mpeg_pcc_tmc13_amd._lib import GpccError
    st = ic.SETTINGS["fd1_sr128"]
    nf = 2048 * 256 + 1500
    fx, fa = synth.random_cloud(nf, seed=77, bits=9, c=1)
    rng = np.random.default_rng(78)
    xyz = np.clip(fx[-1500:] + rng.integers(-1, 2, (1500, 3)), 0, 511).astype(np.int32)
    attrs = np.clip(fa[-1500:] + rng.integers(-6, 7, (1500, 1)), 0, 255).astype(np.int32)
    batch = [(xyz, attrs, np.ascontiguousarray(fx, np.int32), np.ascontiguousarray(fa, np.int32))]
    want = ic.oracle(False, *batch[0], st["search_range"], st["frame_distance"], st["qp"], st["direct"])
    hits = want["frame_hits"]
    assert len(hits) and hits.max() >= 2048 * 256, "no neighbour beyond the first grid's worth of the frame"
    got = dev_batch(ctx, False, True, batch, st)[0]
    np.testing.assert_array_equal(got[0], want["values"])
    np.testing.assert_array_equal(got[1], want["recon"])
    bad = fx.astype(np.int32).copy()
    bad[-1] = (3, 1 << 21, 3)
    with pytest.raises(GpccError) as e:
        dev_batch(ctx, False, True, [(xyz, attrs, bad, batch[0][3])], st)
    assert e.value.code == GPCC_ERR_INVALID_ARG and "2^21" in str(e.value)
    ctx.synchronize()


@pytest.mark.parametrize("predicting", [False, True])
def test_device_tier_frame_coordinate_outside_the_domain(ctx, predicting):
    """a frame coordinate of 2^21 is found on the device: GPCC_ERR_INVALID_ARG from the call (it waits for its slices)
    or from the next synchronisation, and the context works afterwards"""
    from mpeg_pcc_tmc13_amd._lib import GpccError
    st = ic.SETTINGS["fd1_sr128"]
    good = [ic.slice_and_frame(65, 64, 990), ic.slice_and_frame(65, 64, 991)]
    xr = good[1][2].copy()
    xr[10] = (3, 1 << 21, 3)
    bad = [good[0], (good[1][0], good[1][1], xr, good[1][3])]
    with pytest.raises(GpccError) as e:
        dev_batch(ctx, predicting, True, bad, st)
    assert e.value.code == GPCC_ERR_INVALID_ARG and "2^21" in str(e.value)
    ctx.synchronize()
    check_batch(ctx, predicting, good, st)
