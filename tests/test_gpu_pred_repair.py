"""The predicting encoder's finish on the MI355X: slices whose whole-slice passes do not settle (noisy lidar-like
reflectance, three direct predictors, low QP -- declined with GPCC_ERR_UNSUPPORTED before) come back GPCC_OK from every
entry that shares launch_pred, bit-exact against the serial oracle (pinned to the reference on this ground by
tests/test_oracle_pred_unsettled.py), whatever GPCC_PRED_REPAIR_AFTER says."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lod_helpers as lh
import pred_repair_cases as pc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def slice40k():
    """the slice, its oracle structure and per QP the oracle's (values, reconstruction)"""
    xyz, attrs, lp = pc.lidar()
    lod = lh.oracle_lod_generate(xyz, lp)
    want = {}
    for qp in pc.UNSETTLED_QPS:
        v, rec, _, _ = lh.oracle_pred(True, pc.params(lod["npl"], lp, qp), lod, attrs=attrs)
        want[qp] = (v, rec)
    return xyz, attrs, lp, lod, want


def _stats(ctx):
    return ctx.pred_pass_stats(), ctx.pred_repair_stats()


@pytest.mark.parametrize("qp", pc.UNSETTLED_QPS)
def test_one_call_entry_finishes_the_unsettled_slices(ctx, slice40k, qp):
    xyz, attrs, lp, lod, want = slice40k
    p0, r0 = _stats(ctx)
    before = ctx.stats()
    pp = pc.params([len(xyz)], lp, qp)
    v, rec, icp, idx = ctx.pred_encode_attr(lp, pp, xyz, attrs)
    np.testing.assert_array_equal(idx, lod["indexes"])
    np.testing.assert_array_equal(v, want[qp][0])
    np.testing.assert_array_equal(rec, want[qp][1])
    np.testing.assert_array_equal(ctx.pred_decode_attr(lp, pc.params([len(xyz)], lp, qp), xyz, v), rec)
    p1, r1 = _stats(ctx)
    print(f"qp {qp}: passes {p1}, repair {r1}")
    assert ctx.stats()["calls_unsupported"] == before["calls_unsupported"]
    assert p1["declined_at_the_limit"] == 0 and p1["slices"] == p0["slices"] + 1
    assert r1["slices"] == r0["slices"] + 1 and r1["walked"] > r0["walked"] and r1["stretches"] > r0["stretches"]
    assert 0 < r1["longest_stretch"] <= len(xyz)


@pytest.mark.parametrize("qp", pc.UNSETTLED_QPS)
def test_host_tier_entries(ctx, slice40k, qp):
    """gpcc_pred_forward on the caller's structure, gpcc_pred_forward_inter on an inter structure of the same slice"""
    xyz, attrs, lp, lod, want = slice40k
    _, r0 = _stats(ctx)
    v, rec, _ = ctx.pred_forward(pc.params(lod["npl"], lp, qp), lod["nc"], lod["ni"], lod["w"].astype(np.int32),
                                 lod["indexes"], attrs)
    np.testing.assert_array_equal(v, want[qp][0])
    np.testing.assert_array_equal(rec, want[qp][1])
    assert ctx.pred_repair_stats()["slices"] == r0["slices"] + 1
    xr, ar = pc.frame_of(xyz, attrs)
    ilod = lh.oracle_lod_generate_inter(xyz, xr, lp, 64, 1)
    pp = pc.params(ilod["npl"], lp, qp)
    wv, wrec, _ = lh.pred_inter(True, pp, ilod, ar, attrs=attrs)
    iv, irec = ctx.pred_inter(True, pp, dict(ilod, w=ilod["w"].astype(np.int32)), ar, attrs=attrs)
    np.testing.assert_array_equal(iv, wv)
    np.testing.assert_array_equal(irec, wrec)
    np.testing.assert_array_equal(ctx.pred_inter(False, pp, dict(ilod, w=ilod["w"].astype(np.int32)), ar, values=iv)[1], irec)
    print(f"qp {qp}: {_stats(ctx)}")
    assert ctx.pred_pass_stats()["declined_at_the_limit"] == 0


def test_device_tier_batch_mixes_settling_and_unsettled_slices(slice40k):
    """gpcc_dev_pred_encode_attr: lanes are contexts of their own; a slice that needs the walk next to slices that
    settle in a few passes, every slice equal to the oracle's"""
    import torch
    from mpeg_pcc_tmc13_amd import context, synth
    xyz, attrs, lp, lod, want = slice40k
    small = []
    for seed in (5, 6):
        x, a = synth.lidar_cloud(6000, seed=seed)
        small.append((x, np.ascontiguousarray((a >> 8) if a.max() > 255 else a, dtype=np.int32)[:, :1]))
    parts = [(small[0], 28), ((xyz, attrs), 10), (small[1], 28), ((xyz, attrs), 4)]
    offsets = np.concatenate([[0], np.cumsum([len(p[0][0]) for p in parts])]).astype(np.int64)
    dev = torch.device("cuda:0")
    d_xyz = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[0][0] for p in parts]), dtype=np.int32)).to(dev)
    d_a = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[0][1] for p in parts]).reshape(-1))).to(dev)
    d_v = torch.zeros_like(d_a)
    ctx = context(0)
    pps = [pc.params([len(p[0][0])], lp, p[1]) for p in parts]
    ctx.dev_pred_attr(True, lp, pps, offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_v.data_ptr(), 1)
    ctx.synchronize()
    got_v, got_rec = d_v.cpu().numpy(), d_a.cpu().numpy()
    ps, rs = _stats(ctx)
    ctx.close()
    print(f"batch: passes {ps}, repair {rs}")
    for i, ((x, a), qp) in enumerate(parts):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if len(x) == len(xyz):
            wv, wrec = want[qp]
        else:
            l = lh.oracle_lod_generate(x, lp)
            wv, wrec, _, _ = lh.oracle_pred(True, pc.params(l["npl"], lp, qp), l, attrs=a)
        np.testing.assert_array_equal(got_v[lo:hi], wv[:, 0], err_msg=f"values of slice {i}")
        np.testing.assert_array_equal(got_rec[lo:hi], wrec[:, 0], err_msg=f"reconstruction of slice {i}")
    assert ps["slices"] == 4 and ps["declined_at_the_limit"] == 0
    assert rs["slices"] == 2 and rs["walked"] > 0   # the two unsettled ones, and only they


def test_both_candidates_of_the_slice_decision(ctx, slice40k):
    """gpcc_pred_encode_attr_rdo: the inter and the intra candidate of the unsettled slice, each equal to the oracle's
    encoder on the oracle's structure, the distortions the sums numpy gives"""
    xyz, attrs, lp, lod, want = slice40k
    xr, ar = pc.frame_of(xyz, attrs)
    ilod = lh.oracle_lod_generate_inter(xyz, xr, lp, 64, 1)
    qp = 10
    wv, wrec, _ = lh.pred_inter(True, pc.params(ilod["npl"], lp, qp), ilod, ar, attrs=attrs)
    src = attrs.copy()
    values, recon, dist = ctx.pred_encode_attr_rdo(lp, lp, pc.params([len(xyz)], lp, qp), xyz, attrs, xr, ar, 64, 1)
    np.testing.assert_array_equal(attrs, src)
    np.testing.assert_array_equal(values[0], wv[:, 0])
    np.testing.assert_array_equal(recon[0], wrec[:, 0])
    np.testing.assert_array_equal(values[1], want[qp][0][:, 0])
    np.testing.assert_array_equal(recon[1], want[qp][1][:, 0])
    np.testing.assert_array_equal(dist, np.abs(recon.astype(np.int64) - src[:, 0]).sum(axis=1))
    if lh.entropy_available():
        # the decision as the reference takes it, from the bytes its own entropy coder needs for these values
        from mpeg_pcc_tmc13_amd.raht import slice_rdo_choose
        n = len(xyz)

        def nbytes(v):
            runs, vals, trailing = ctx.zero_run_pack(v, n, 1, 0)
            return len(lh.ref_entropy_encode_bins(ctx.binarise_symbols(runs, vals, trailing, 1), n))

        def obytes(v):
            runs, vals, trailing = lh.oracle_zero_run_pack(v, n, 1, 0)
            return len(lh.ref_entropy_encode_bins(lh.oracle_binarise_symbols(runs, vals, trailing, 1), n))

        got = [nbytes(values[k]) for k in (0, 1)]
        assert got == [obytes(wv[:, 0]), obytes(want[qp][0][:, 0])]
        odist = [int(np.abs(w.astype(np.int64)[:, 0] - src[:, 0]).sum()) for w in (wrec, want[qp][1])]
        assert slice_rdo_choose(dist[0], got[0], dist[1], got[1], qp - 4) == slice_rdo_choose(odist[0], got[0], odist[1], got[1], qp - 4)


def test_sharded_entry_on_one_device(slice40k):
    """gpcc_multi_pred_encode_attr, all shards on device 0"""
    from mpeg_pcc_tmc13_amd.raht import MultiContext
    xyz, attrs, lp, lod, want = slice40k
    qps = list(pc.UNSETTLED_QPS)
    n = len(xyz)
    offsets = np.array([0, n, 2 * n], dtype=np.int64)
    blocks = [pc.params([0], lp, qp) for qp in qps]
    mc = MultiContext([0, 0])
    v, rec, side, idx = mc.lod_encode_attr(True, lp, blocks, offsets, np.concatenate([xyz, xyz]), np.concatenate([attrs, attrs]))
    mc.close()
    for i, qp in enumerate(qps):
        np.testing.assert_array_equal(v[i * n:(i + 1) * n], want[qp][0], err_msg=f"shard {i}")
        np.testing.assert_array_equal(rec[i * n:(i + 1) * n], want[qp][1], err_msg=f"shard {i}")


@pytest.mark.parametrize("qp", [4, 10])
def test_one_million_points(ctx, qp):
    xyz, attrs, lp = pc.lidar(1000000)
    lod = lh.oracle_lod_generate(xyz, lp)
    wv, wrec, _, _ = lh.oracle_pred(True, pc.params(lod["npl"], lp, qp), lod, attrs=attrs)
    _, r0 = _stats(ctx)
    v, rec, _, idx = ctx.pred_encode_attr(lp, pc.params([len(xyz)], lp, qp), xyz, attrs)
    p1, r1 = _stats(ctx)
    print(f"1M qp {qp}: passes {p1}, repair {r1}")
    np.testing.assert_array_equal(idx, lod["indexes"])
    np.testing.assert_array_equal(v, wv)
    np.testing.assert_array_equal(rec, wrec)
    assert p1["declined_at_the_limit"] == 0 and r1["slices"] == r0["slices"] + 1


def test_no_allocation_in_the_steady_state(slice40k):
    """a context that has coded the slice once allocates nothing when it codes it again, the walk included (the
    walk's lists and marks live in the rate recurrence's scratch, which the slice carve already accounts for)"""
    from mpeg_pcc_tmc13_amd import _lib, context
    xyz, attrs, lp, lod, want = slice40k

    def events(c):
        out = (C.c_longlong * 4)()
        _lib.load().gpcc_debug_alloc_events.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        assert _lib.load().gpcc_debug_alloc_events(c._h, out) == 0
        return list(out)

    c = context(0)
    c.reserve(len(xyz), 1, 1)
    c.pred_encode_attr(lp, pc.params([len(xyz)], lp, 10), xyz, attrs)
    ev0, ws = events(c), c.workspace_bytes()
    for qp in pc.UNSETTLED_QPS:
        v, rec, _, _ = c.pred_encode_attr(lp, pc.params([len(xyz)], lp, qp), xyz, attrs)
        np.testing.assert_array_equal(v, want[qp][0])
    assert c.pred_repair_stats()["slices"] == 3
    assert events(c) == ev0 and c.workspace_bytes() == ws
    c.close()


def test_result_does_not_depend_on_the_switch_point(tmp_path, slice40k):
    """GPCC_PRED_REPAIR_AFTER = 1 (the whole slice walked) and 8, a fresh process each: identical output, the oracle's"""
    xyz, attrs, lp, lod, want = slice40k
    outs = {}
    for after in (1, 8):
        path = str(tmp_path / f"after{after}.npz")
        env = dict(os.environ, GPCC_PRED_REPAIR_AFTER=str(after))
        r = subprocess.run([sys.executable, os.path.join(HERE, "pred_repair_worker.py"), path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[after] = dict(np.load(path))
        print(f"after {after}: passes {outs[after]['pass_stats']}, repair {outs[after]['repair_stats']}")
    for k in outs[1]:
        if not k.endswith("_stats"):
            np.testing.assert_array_equal(outs[1][k], outs[8][k], err_msg=k)
    for qp in pc.UNSETTLED_QPS:
        np.testing.assert_array_equal(outs[1][f"v{qp}"], want[qp][0])
        np.testing.assert_array_equal(outs[1][f"rec{qp}"], want[qp][1])
    n = len(xyz)
    assert outs[1]["pass_stats"][2] == 1 and outs[1]["repair_stats"][0] == 3 and outs[1]["repair_stats"][1] == 3 * n
    assert outs[8]["pass_stats"][2] <= 8 and outs[8]["pass_stats"][3] == 0 and outs[8]["repair_stats"][1] > 0
