"""GPU parity of the spherical-domain attribute positions (gpcc_attr_to_spherical / gpcc_dev_attr_to_spherical)
with the reference's convertXyzToRpl + offsetAndScale: every case of tests/golden/spherical_golden.npz through the
host entry and through the device entry -- positions, bounding boxes, digests --, the ragged 300-slice batch in one
device call, the in-place form in both tiers, a chain that stays in HBM up to the RAHT coefficients, and a point
outside the domain (an error code, not a fault).  Bit-exact, no tolerance."""
import numpy as np
import pytest

import spherical_cases as sc

pytestmark = pytest.mark.gpu

UNIT = dict(scale=(256, 256, 256), mode=1, min_pos=(0, 0, 0))  # offsetAndScale as the identity: the unscaled result
GPCC_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


def host_run(ctx, c, out=None):
    """one host call per slice of the case"""
    off = c["offsets"]
    pos, boxes = [], []
    for s in range(len(off) - 1):
        p, b = ctx.attr_to_spherical(sc.params(c), c["xyz"][off[s]:off[s + 1]], out=out)
        pos.append(p)
        boxes.append(b.reshape(6))
    return np.concatenate(pos), np.stack(boxes)


def dev_run(ctx, c, in_place=False, misalign=0, bbox=True):
    """the whole batch in one device call; misalign: the arrays start that many int32 behind torch's allocation"""
    import torch
    dev = torch.device("cuda:0")
    n = len(c["xyz"])
    d_in = torch.zeros(3 * n + misalign, dtype=torch.int32, device=dev)
    d_in[misalign:] = torch.from_numpy(np.ascontiguousarray(c["xyz"]).reshape(-1)).to(dev)
    d_out = d_in if in_place else torch.full((3 * n + misalign,), -1, dtype=torch.int32, device=dev)
    d_box = torch.full((6 * (len(c["offsets"]) - 1),), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.dev_attr_to_spherical(sc.params(c), c["offsets"], d_in.data_ptr() + 4 * misalign, d_out.data_ptr() + 4 * misalign,
                              d_box.data_ptr() if bbox else None)
    ctx.synchronize()
    return d_out[misalign:].cpu().numpy().reshape(-1, 3), d_box.cpu().numpy().reshape(-1, 6)


_unscaled = {}


def entry_input(ctx, c):
    """the Cartesian cloud, or -- convert = 0 -- the unscaled result of the case it derives from, computed once by the
    host entry and pinned to that case's digest"""
    if c["convert"]:
        return c["xyz"]
    if c["of"] not in _unscaled:
        base = sc.case(c["of"])
        rpl = host_run(ctx, dict(base, **UNIT))[0]
        assert sc.digest(rpl) == base["rpl_sha"]
        _unscaled[c["of"]] = rpl
    return _unscaled[c["of"]]


def check(c, pos, bbox):
    np.testing.assert_array_equal(bbox, c["bbox"])
    if "pos" in c:
        np.testing.assert_array_equal(pos, c["pos"])
    assert sc.digest(pos) == c["pos_sha"]


@pytest.mark.parametrize("name", [n for n in sc.NAMES if n != "ragged300"])
def test_case_matches_the_reference_in_both_tiers(name, ctx):
    c = sc.case(name)
    c["xyz"] = entry_input(ctx, c)
    check(c, *host_run(ctx, c))
    check(c, *dev_run(ctx, c))
    if c["convert"] and c["bbox"].max() < (1 << 21):
        # the unscaled (r, phi, laser) as well (all cases but "corners", whose radii a unit scale leaves too large)
        rpl, bbox = dev_run(ctx, dict(c, **UNIT))
        np.testing.assert_array_equal(bbox, c["bbox"])
        if "rpl" in c:
            np.testing.assert_array_equal(rpl, c["rpl"])
        assert sc.digest(rpl) == c["rpl_sha"]


def test_ragged_batch_in_one_device_call(ctx):
    """300 slices of 1..60 points with disjoint boxes: a reduction that bleeds across slices shows in the boxes and,
    through the minima, in every position"""
    c = sc.case("ragged300")
    pos, bbox = dev_run(ctx, c)
    check(c, pos, bbox)
    hpos, hbox = host_run(ctx, c)
    np.testing.assert_array_equal(hpos, pos)
    np.testing.assert_array_equal(hbox, bbox)
    # the boxes are workspace when the caller passes none
    np.testing.assert_array_equal(dev_run(ctx, c, bbox=False)[0], pos)


@pytest.mark.parametrize("name", ["size_5", "size_257", "hand_synth64", "ragged300", "lidar_2000_s1_sph_min2",
                                  "lidar_200000_s21"])
def test_in_place_in_both_tiers(name, ctx):
    c = sc.case(name)
    c["xyz"] = entry_input(ctx, c)
    check(c, *dev_run(ctx, c, in_place=True))
    # ... and arrays that do not start on a 16-byte boundary (every point takes the scalar path)
    check(c, *dev_run(ctx, c, in_place=True, misalign=1))
    check(c, *dev_run(ctx, c, misalign=3))
    if len(c["offsets"]) == 2:
        buf = np.ascontiguousarray(c["xyz"]).copy()
        pos, bbox = ctx.attr_to_spherical(sc.params(c), buf, out=buf)
        assert pos is buf
        check(c, buf, bbox.reshape(1, 6))


def test_chain_stays_in_hbm(ctx):
    """xyz -> spherical positions -> Morton order -> RAHT coefficients without leaving the device, against the same
    sort and transform fed with the reference's positions"""
    import torch
    from mpeg_pcc_tmc13_amd import raht_params, synth
    c = sc.case("lidar_200000_s21")
    _, refl = synth.lidar_cloud(200000, seed=21)
    n = len(c["xyz"])
    assert len(refl) == n
    want_pos, _ = host_run(ctx, c)
    assert sc.digest(want_pos) == c["pos_sha"]  # (the fixture's positions)
    dev = torch.device("cuda:0")
    p = raht_params(qp=34)
    d_attr = torch.from_numpy(refl.reshape(-1)).to(dev)

    def sort_and_transform(d_pos):
        d_m = torch.zeros(n, dtype=torch.int64, device=dev)
        d_o = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.dev_attr_morton_sort(c["offsets"], d_pos.data_ptr(), d_m.data_ptr(), d_o.data_ptr())
        ctx.synchronize()
        d_a = d_attr[d_o.long()].contiguous()
        d_c = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.dev_raht_forward(p, c["offsets"], d_m.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), 1)
        ctx.synchronize()
        return d_m.cpu().numpy(), d_o.cpu().numpy(), d_c.cpu().numpy(), d_a.cpu().numpy()

    d_xyz = torch.from_numpy(c["xyz"].reshape(-1)).to(dev)
    torch.cuda.synchronize()
    ctx.dev_attr_to_spherical(sc.params(c), c["offsets"], d_xyz.data_ptr(), d_xyz.data_ptr())  # (no host wait here)
    got = sort_and_transform(d_xyz)
    want = sort_and_transform(torch.from_numpy(want_pos.reshape(-1)).to(dev))
    for g, w, what in zip(got, want, ("codes", "order", "coefficients", "reconstruction")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    assert np.all(np.diff(got[0]) >= 0) and np.count_nonzero(got[2]) > 0


def test_a_point_outside_the_domain_is_an_error_code(ctx):
    from mpeg_pcc_tmc13_amd._lib import GpccError
    c = sc.case("size_257")
    bad = dict(c, xyz=c["xyz"].copy())
    bad["xyz"][200] = c["origin"] + np.array([0, 1 << 22, 0])
    # device tier: the call is enqueued; the next synchronisation reports it, once
    with pytest.raises(GpccError) as e:
        dev_run(ctx, bad)
    assert e.value.code == GPCC_ERR_INVALID_ARG and "outside the domain" in str(e.value)
    ctx.synchronize()
    # host tier: refused, pos_out and the box untouched
    out = np.full((257, 3), -7, np.int32)
    with pytest.raises(GpccError) as e:
        ctx.attr_to_spherical(sc.params(bad), bad["xyz"], out=out)
    assert e.value.code == GPCC_ERR_INVALID_ARG and "outside the domain" in str(e.value)
    assert (out == -7).all()
    # a scaled coordinate outside [0, 2^21) likewise
    with pytest.raises(GpccError) as e:
        ctx.attr_to_spherical(sc.params(dict(c, scale=(256 * 16, 256, 256))), c["xyz"], out=out)
    assert e.value.code == GPCC_ERR_INVALID_ARG and (out == -7).all()
    # the context is as good as before
    check(c, *host_run(ctx, c))
    check(c, *dev_run(ctx, c))
