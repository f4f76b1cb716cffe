"""The predicting encoder's finish under the CPU wavefront emulator: the library's whole-slice passes, then
pred_walk_kernel over the decisions they leave open, driven by the library's own host-side decisions
(csrc/pred_repair.hpp), against the serial oracle.  No GPU needed."""
import numpy as np
import pytest

import emu_pred_repair_loader as er
import lod_helpers as lh

NEVER = 64  # GPCC_PRED_REPAIR_AFTER beyond the passes the small slices below take: the walk is not reached


def lidar_case(n, seed=21, refl_noise=24):
    from mpeg_pcc_tmc13_amd import lod_params, synth
    xyz, attrs = synth.lidar_cloud(n, seed=seed, refl_noise=refl_noise)
    if attrs.max() > 255:
        attrs = attrs >> 8
    lp = lod_params(lifting=False, intra_range=64)
    lp.intra_lod_prediction_skip_layers = 0
    return xyz, attrs, lp


def refl_params(lod, lp, qp, direct=3, avg_disabled=False, qnw=(0, 0, 0)):
    from mpeg_pcc_tmc13_amd import pred_params
    return pred_params(lod["npl"], qp=qp, chroma_offset=0, bitdepth=8, threshold=4, direct=direct, icp=False,
                       avg_disabled=avg_disabled, quant_neigh_weight=qnw, max_levels=lp.num_detail_levels_minus1 + 1)


@pytest.mark.parametrize("qp", [10, 4])
def test_slices_whose_passes_do_not_settle_are_finished_by_the_walk(qp):
    """40 000 noisy lidar points, three direct predictors: 64 whole-slice passes do not settle these two (the
    encoder declined them).  With the walk they equal the oracle, and the walk has run."""
    xyz, attrs, lp = lidar_case(40000)
    lod = lh.oracle_lod_generate(xyz, lp)
    pp = refl_params(lod, lp, qp)
    v, rec, _, _ = lh.oracle_pred(True, pp, lod, attrs=attrs)
    ev, erec, _, st = er.encode(pp, lod, attrs)
    print(f"qp {qp}: {st}")
    np.testing.assert_array_equal(ev, v)
    np.testing.assert_array_equal(erec, rec)
    assert st["walked"] > 0 and st["differences"] > 0 and st["passes"] == er.after_from_text(None)


def _switch_independent(pp, lod, attrs, v, rec, icp=None, attrs_ref=None):
    outs = []
    for after in (1, 3, NEVER):
        ev, erec, eicp, st = er.encode(pp, lod, attrs, attrs_ref=attrs_ref, repair_after=after)
        print(f"after {after}: {st}")
        np.testing.assert_array_equal(ev, v, err_msg=f"values, switch after {after}")
        np.testing.assert_array_equal(erec, rec, err_msg=f"reconstruction, switch after {after}")
        if icp is not None:
            np.testing.assert_array_equal(eicp, icp)
        outs.append(st)
    # after one pass everything counts as different: the whole slice is walked, once
    assert outs[0]["passes"] == 1 and outs[0]["walked"] == len(attrs) and outs[0]["stretches"] == 1
    assert outs[1]["passes"] == 3
    assert outs[2]["walked"] == 0 and outs[2]["passes"] < NEVER
    return outs


@pytest.mark.parametrize("avg_disabled", [False, True])
def test_result_does_not_depend_on_the_switch_point_lidar(avg_disabled):
    xyz, attrs, lp = lidar_case(3000)
    lod = lh.oracle_lod_generate(xyz, lp)
    pp = refl_params(lod, lp, 10, avg_disabled=avg_disabled, qnw=(16, 8, 4) if avg_disabled else (0, 0, 0))
    v, rec, _, _ = lh.oracle_pred(True, pp, lod, attrs=attrs)
    outs = _switch_independent(pp, lod, attrs, v, rec)
    assert 0 < outs[1]["walked"] < len(attrs)


def test_result_does_not_depend_on_the_switch_point_colour():
    """dense colour, three components, inter-component prediction on, several LoDs"""
    from mpeg_pcc_tmc13_amd import lod_params, pred_params, synth
    xyz, attrs = synth.dense_cloud(2500, seed=3, bits=7)
    lp = lod_params(lifting=False, intra_range=64)
    lp.intra_lod_prediction_skip_layers = 0
    lod = lh.oracle_lod_generate(xyz, lp)
    for qp, chroma in ((10, 0), (22, 2)):
        pp = pred_params(lod["npl"], qp=qp, chroma_offset=chroma, bitdepth=8, threshold=16, direct=3, icp=True,
                         quant_neigh_weight=(0, 0, 0), max_levels=lp.num_detail_levels_minus1 + 1)
        v, rec, icp, _ = lh.oracle_pred(True, pp, lod, attrs=attrs)
        _switch_independent(pp, lod, attrs, v, rec, icp=icp)


def test_result_does_not_depend_on_the_switch_point_inter():
    """neighbours in a reference frame"""
    rng = np.random.default_rng(7)
    xyz, attrs, lp = lidar_case(2500, seed=61)
    keep = rng.random(len(xyz)) > 0.1
    xr = np.clip(xyz + rng.integers(-2, 3, size=xyz.shape), 0, None)[keep].astype(np.int32)
    ar = np.clip(attrs + rng.integers(-6, 7, size=attrs.shape), 0, 255)[keep].astype(np.int32)
    lod = lh.oracle_lod_generate_inter(xyz, xr, lp, 64, 1)
    assert lod["ref"].any()
    for avg_disabled in (False, True):
        pp = refl_params(lod, lp, 7, avg_disabled=avg_disabled)
        v, rec, _ = lh.pred_inter(True, pp, lod, ar, attrs=attrs)
        _switch_independent(pp, lod, attrs, v, rec, attrs_ref=ar)


@pytest.mark.parametrize("n", [1, 5])
def test_tiny_slices(n):
    from mpeg_pcc_tmc13_amd import lod_params, synth
    xyz, attrs = synth.random_cloud(n, seed=2, bits=3, c=1)
    lp = lod_params(lifting=False, intra_range=64)
    lp.intra_lod_prediction_skip_layers = 0
    lod = lh.oracle_lod_generate(xyz, lp)
    pp = refl_params(lod, lp, 4)
    v, rec, _, _ = lh.oracle_pred(True, pp, lod, attrs=attrs)
    for after in (1, 2, NEVER):
        ev, erec, _, st = er.encode(pp, lod, attrs, repair_after=after)
        np.testing.assert_array_equal(ev, v)
        np.testing.assert_array_equal(erec, rec)
        assert st["walked"] == (n if after == 1 else 0)


def test_one_direct_predictor_and_a_walk_that_ends_at_the_last_predictor():
    xyz, attrs, lp = lidar_case(3000)
    lod = lh.oracle_lod_generate(xyz, lp)
    pp = refl_params(lod, lp, 10, direct=1)
    v, rec, _, _ = lh.oracle_pred(True, pp, lod, attrs=attrs)
    _switch_independent(pp, lod, attrs, v, rec)
    # the only difference the walk starts from is the LAST predictor: cut the slice behind the first difference
    # (everything is causal in coding order, so the passes of the cut slice leave the same difference there)
    pp = refl_params(lod, lp, 10)
    _, _, _, st = er.encode(pp, lod, attrs, repair_after=2)
    cut = st["first"] + 1
    assert 1 < cut < len(attrs)
    order = np.asarray(lod["indexes"])
    sub = dict(nc=lod["nc"][:cut].copy(), ni=lod["ni"][:cut].copy(), w=lod["w"][:cut].copy(),
               indexes=np.argsort(np.argsort(order[:cut])).astype(np.int32),
               npl=np.minimum(np.asarray(lod["npl"]), cut).astype(np.int32))
    a = attrs[np.sort(order[:cut])]
    ppc = refl_params(sub, lp, 10)
    v, rec, _, _ = lh.oracle_pred(True, ppc, sub, attrs=a)
    ev, erec, _, st = er.encode(ppc, sub, a, repair_after=2)
    np.testing.assert_array_equal(ev, v)
    np.testing.assert_array_equal(erec, rec)
    assert st["first"] == st["last"] == cut - 1 and st["walked"] == 1


def test_switch_from_its_environment_text():
    d = er.after_from_text(None)
    assert 1 <= d <= 64
    assert [er.after_from_text(t) for t in ("", "x", "0", "-3", "3x")] == [d] * 5
    assert er.after_from_text("1") == 1 and er.after_from_text("12") == 12 and er.after_from_text("1000") == 64
