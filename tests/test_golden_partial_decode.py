"""The fixture of the partial (spatially scalable) decode of scalable-lifting slices
(tests/golden/partial_decode_golden.npz, from the compiled reference): well-formed, its m = 0 case equal to the
pinned whole-slice path (CPU oracle), and the quantisation weights of a partially decoded slice -- the device
kernel under the CPU wavefront emulator -- against a numpy restatement of computeQuantizationWeightsScalable."""
import numpy as np
import pytest

import emu_lod_partial_loader as el
import lod_helpers as lh
import oracle_loader as ol
import partial_decode_cases as pc


def test_fixture_lists_every_case():
    assert [str(n) for n in pc.golden()["names"]] == pc.NAMES
    assert {pc.case(n)["m"] for n in pc.NAMES} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", pc.NAMES)
def test_fixture_is_well_formed(name):
    c = pc.case(name)   # (regenerates the cloud and checks N and P against the fixture)
    P, m, N = len(c["xyz"]), c["m"], c["N"]
    assert 0 < P <= N and (m > 0 or P == N)
    npl = c["npl"]
    assert npl[-1] == P and np.all(np.diff(npl) >= 0) and len(npl) <= 21 - m
    # the cloud of a decode that stopped m levels early: nodes of size 2^m, one point each
    assert len(np.unique(c["xyz"] >> m, axis=0)) == P
    if m:
        low = c["xyz"] & ((1 << m) - 1)
        assert np.all((low == 0) | (low == 1 << (m - 1)))
    assert c["coeffs"].shape[0] == P and c["coeffs"].shape[1] in (1, 3)
    assert len(c["lod_sha"]) == 64 and len(c["attrs_sha"]) == 64
    assert (c["lod"] is not None) == (name in pc.FULL)


@pytest.mark.parametrize("name", pc.FULL)
def test_full_cases_hold_a_structure(name):
    """the cases stored in full: a LoD structure, and the digests are those of what is stored"""
    c = pc.case(name)
    lod, P, npl = c["lod"], len(c["xyz"]), c["npl"]
    assert sorted(lod["indexes"]) == list(range(P))
    nc, ni = lod["nc"], lod["ni"]
    assert nc.min() >= 0 and nc.max() <= 3 and nc[0] == 0
    live = np.arange(3)[None, :] < nc[:, None]
    # a neighbour precedes its predictor's level of detail
    start = np.concatenate([[0], npl])[np.searchsorted(npl, np.arange(P), side="right")]
    assert np.all(ni[live] < np.broadcast_to(start[:, None], ni.shape)[live])
    assert np.all(lod["w"][live] > 0) and np.all(lod["w"].sum(axis=1)[nc > 0] == 256)
    assert c["attrs"].shape == c["coeffs"].shape and c["attrs"].min() >= 0 and c["attrs"].max() <= 255
    assert pc.lod_digest(lod) == c["lod_sha"] and pc.attrs_digest(c["attrs"]) == c["attrs_sha"]


def test_m0_case_is_the_whole_slice_path():
    """the generator cross-checked: with m = 0 the fixture is what the pinned oracle computes"""
    c = pc.case("dense_m0")
    lp = pc.lod_params_of(c)
    want = lh.oracle_lod_generate(c["xyz"], lp)
    pc.assert_lod(want, c, "dense_m0")
    lf = pc.lift_params_of(c)
    rec = lh.lift(ol.oracle(), False, lf, want, np.zeros_like(c["coeffs"]), coeffs=c["coeffs"], lcp=c["lcp"])[1]
    pc.assert_attrs(rec, c, "dense_m0")


@pytest.mark.parametrize("name", pc.NAMES)
def test_partial_quant_weights_kernel_vs_numpy(name):
    """item 3 of the partial decode: numerator N, no unit weight for the finest level when m > 0"""
    c = pc.case(name)
    npl, P = c["npl"], len(c["xyz"])
    got = el.quant_weights(P, c["m"], c["N"], npl)
    np.testing.assert_array_equal(got, pc.quant_weights_numpy(npl, c["N"], c["m"]))
    if c["m"]:
        # not what a whole slice of P points would get: the finest level carries N / P, the rest N / size
        assert got[-1] == (c["N"] // P) << 8
        assert got[0] == c["N"] << 8


def test_partial_quant_weights_m0_is_the_whole_slice_rule():
    npl = np.array([1, 9, 70, 400], np.int32)
    got = el.quant_weights(400, 0, 400, npl)
    want = np.concatenate([[400 << 8], np.full(8, (400 // 9) << 8), np.full(61, (400 // 70) << 8), np.full(330, 256)])
    np.testing.assert_array_equal(got, want.astype(np.uint64))
