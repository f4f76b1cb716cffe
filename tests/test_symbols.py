"""Zero-run formation of the coefficient stream (the non-arithmetic part of the
reference's entropy loops, AttributeEncoder.cpp:1279-1291 / 1347-1362 RAHT,
:1458-1474 / 1617-1633 lifting) pinned at BITSTREAM level: the symbols are fed
to the reference's own PCCResidualsEncoder and the bytes must equal the
arithmetic-coded part of the payload AttributeEncoder::encode writes for the
same slice.  CPU: oracle symbols from reference coefficients.  GPU: the device
transform + device symbol packing -> bitstream identical to the reference
operator."""
import numpy as np
import pytest

import conftest  # noqa: F401
import lod_helpers as lh
import oracle_loader as ol

needs_ref = pytest.mark.skipif(not (ol.ref_available() and lh.entropy_available()),
                               reason="compiled reference / entropy harness absent")

RAHT_CASES = [("dense", 20000, 8, 34, -1), ("dense", 6000, 7, 22, 0), ("lidar", 30000, 0, 34, 0),
              ("random", 1500, 5, 40, -2), ("random", 1, 3, 34, 0)]


def cloud(kind, n, bits):
    from mpeg_pcc_tmc13_amd import synth
    if kind == "dense":
        return synth.dense_cloud(n, seed=61, bits=bits)
    if kind == "lidar":
        return synth.lidar_cloud(n, seed=61)
    return synth.random_cloud(n, seed=61, bits=bits)


def reference_ac_bytes(lp, transform, rp, qp, chroma, bitdepth, lcp, xyz, attrs):
    payload, rec_enc, rec_dec = lh.ref_operator_roundtrip(lp, transform, rp, qp, chroma, bitdepth, lcp, xyz, attrs)
    np.testing.assert_array_equal(rec_enc, rec_dec)
    return payload[lh.ref_last_abh_size():], rec_enc


@needs_ref
@pytest.mark.parametrize("case", RAHT_CASES, ids=lambda c: f"{c[0]}-{c[1]}-qp{c[3]}")
def test_raht_symbols_give_the_reference_bitstream(case):
    from mpeg_pcc_tmc13_amd import lod_params, raht_params
    kind, n, bits, qp, chroma = case
    xyz, attrs = cloud(kind, n, bits)
    c = attrs.shape[1]
    bitdepth = 8 if c == 3 else 16
    rp = raht_params(qp=qp, chroma_offset=chroma)
    want, want_rec = reference_ac_bytes(lod_params(), 0, rp, qp, chroma, bitdepth, False, xyz, attrs)
    r = ol.ref()
    morton, order = r.morton_sort(xyz)
    co, rec = r.raht_forward(rp, morton, attrs[order])
    runs, vals, trailing = lh.oracle_zero_run_pack(co, len(xyz), c, planar=True)
    assert lh.ref_entropy_encode_symbols(c, len(xyz), runs, vals, trailing) == want
    out = np.zeros_like(attrs)
    out[order] = np.clip(rec, 0, (1 << bitdepth) - 1)
    np.testing.assert_array_equal(out, want_rec)


@needs_ref
@pytest.mark.parametrize("kind,n,bits", [("dense", 8000, 7), ("lidar", 9000, 0)])
def test_lifting_symbols_give_the_reference_bitstream(kind, n, bits):
    from mpeg_pcc_tmc13_amd import lift_params, lod_params, raht_params
    xyz, attrs = cloud(kind, n, bits)
    c = attrs.shape[1]
    bitdepth = 8 if c == 3 else 16
    lp = lod_params()
    want, want_rec = reference_ac_bytes(lp, 2, raht_params(), 34, 0, bitdepth, c == 3, xyz, attrs)
    lod = lh.ref_lod_generate(xyz, lp)
    lf = lift_params(lod["npl"], qp=34, chroma_offset=0, lcp=(c == 3), bitdepth=bitdepth)
    co, rec, lcp = lh.lift(ol.ref(), True, lf, lod, attrs)
    runs, vals, trailing = lh.oracle_zero_run_pack(co, len(xyz), c, planar=False)
    assert lh.ref_entropy_encode_symbols(c, len(xyz), runs, vals, trailing) == want
    np.testing.assert_array_equal(rec, want_rec)


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("case", RAHT_CASES + [("dense", 300000, 10, 34, -1)], ids=lambda c: f"{c[0]}-{c[1]}-qp{c[3]}")
def test_device_raht_bitstream_identical_to_reference_operator(case, ctx):
    """xyz + attributes -> device slice driver (sort, RAHT with the reference's
    default flags, clip, scatter) -> device zero-run packing -> the reference's
    arithmetic coder: the bytes equal the reference operator's payload."""
    from mpeg_pcc_tmc13_amd import lod_params, raht_params
    kind, n, bits, qp, chroma = case
    xyz, attrs = cloud(kind, n, bits)
    c = attrs.shape[1]
    bitdepth = 8 if c == 3 else 16
    rp = raht_params(qp=qp, chroma_offset=chroma)
    want, want_rec = reference_ac_bytes(lod_params(), 0, rp, qp, chroma, bitdepth, False, xyz, attrs)
    co, rec = ctx.raht_encode_attr(rp, xyz, attrs, bitdepth)
    runs, vals, trailing = ctx.zero_run_pack(co, len(xyz), c, planar=True)
    o_runs, o_vals, o_tr = lh.oracle_zero_run_pack(co, len(xyz), c, planar=True)
    np.testing.assert_array_equal(runs, o_runs)
    np.testing.assert_array_equal(vals, o_vals)
    assert trailing == o_tr
    assert lh.ref_entropy_encode_symbols(c, len(xyz), runs, vals, trailing) == want
    np.testing.assert_array_equal(rec, want_rec)
    # the one-call form: symbols straight from the device
    p_runs, p_vals, p_tr, p_rec = ctx.raht_encode_attr_packed(rp, xyz, attrs, bitdepth)
    np.testing.assert_array_equal(p_runs, runs)
    np.testing.assert_array_equal(p_vals, vals)
    assert p_tr == trailing
    np.testing.assert_array_equal(p_rec, rec)


@pytest.mark.gpu
def test_device_packed_symbols_past_the_partition_shape_change(ctx):
    """the one-call form carves its own workspace for the zero-run kernels: its symbols equal those of the
    two-call form and the oracle's at 1 048 577 points, where the look-back partition first runs with empty
    trailing workgroups"""
    from mpeg_pcc_tmc13_amd import raht_params, synth
    n = 1048577
    xyz, attrs = synth.random_cloud(n, seed=61, bits=10, c=1)
    rp = raht_params(qp=34, chroma_offset=0)
    co, rec = ctx.raht_encode_attr(rp, xyz, attrs, 16)
    runs, vals, trailing = ctx.zero_run_pack(co, n, 1, planar=True)
    o_runs, o_vals, o_tr = lh.oracle_zero_run_pack(co, n, 1, planar=True)
    np.testing.assert_array_equal(runs, o_runs)
    np.testing.assert_array_equal(vals, o_vals)
    assert trailing == o_tr and 0 < len(runs) < n
    p_runs, p_vals, p_tr, p_rec = ctx.raht_encode_attr_packed(rp, xyz, attrs, 16)
    np.testing.assert_array_equal(p_runs, runs)
    np.testing.assert_array_equal(p_vals, vals)
    assert p_tr == trailing
    np.testing.assert_array_equal(p_rec, rec)


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("kind,n,bits", [("dense", 8000, 7), ("lidar", 9000, 0), ("dense", 200000, 10)])
def test_device_lifting_bitstream_identical_to_reference_operator(kind, n, bits, ctx):
    from mpeg_pcc_tmc13_amd import lift_params, lod_params, raht_params
    xyz, attrs = cloud(kind, n, bits)
    c = attrs.shape[1]
    bitdepth = 8 if c == 3 else 16
    lp = lod_params()
    want, want_rec = reference_ac_bytes(lp, 2, raht_params(), 34, 0, bitdepth, c == 3, xyz, attrs)
    lf = lift_params([len(xyz)], qp=34, chroma_offset=0, lcp=(c == 3), bitdepth=bitdepth)
    co, rec, lcp, idx = ctx.lift_encode_attr(lp, lf, xyz, attrs)
    runs, vals, trailing = ctx.zero_run_pack(co, len(xyz), c, planar=False)
    assert lh.ref_entropy_encode_symbols(c, len(xyz), runs, vals, trailing) == want
    np.testing.assert_array_equal(rec, want_rec)
