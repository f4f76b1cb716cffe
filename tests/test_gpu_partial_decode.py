"""GPU parity of the partial (spatially scalable) decode of scalable-lifting slices through the C ABI
(gpcc_lod_build_partial, gpcc_lift_inverse_partial, gpcc_lift_decode_attr_partial,
gpcc_dev_lift_decode_attr_partial) against the committed results of the compiled reference
(tests/golden/partial_decode_golden.npz: AttributeLods::generate and AttributeDecoder::decode with
minGeomNodeSizeLog2 = m > 0), and of the new entries against the existing ones where they must coincide.
Bit-exact."""
import numpy as np
import pytest

import partial_decode_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", pc.NAMES)
def test_lod_build_partial_vs_reference(name, ctx):
    c = pc.case(name)
    got = ctx.lod_build(pc.lod_params_of(c), c["xyz"], min_geom_node_size_log2=c["m"], geom_num_points=c["N"])
    pc.assert_lod(got, c, name)


@pytest.mark.parametrize("name", pc.NAMES)
def test_lift_inverse_partial_vs_reference(name, ctx):
    """the reference's predictors + the first P coefficients -> the reference's decoded attributes (predictors:
    the stored ones where the fixture holds them in full, else the device's, checked to be the reference's)"""
    c = pc.case(name)
    lod = c["lod"]
    if lod is None:
        lod = ctx.lod_build(pc.lod_params_of(c), c["xyz"], min_geom_node_size_log2=c["m"], geom_num_points=c["N"])
        pc.assert_lod(lod, c, name)
    rec = ctx.lift_inverse(pc.lift_params_of(c), lod["nc"], lod["ni"], lod["w"], lod["indexes"], c["coeffs"],
                           lcp=c["lcp"], min_geom_node_size_log2=c["m"], geom_num_points=c["N"])
    pc.assert_attrs(rec, c, name)


@pytest.mark.parametrize("name", pc.NAMES)
def test_lift_decode_attr_partial_vs_reference(name, ctx):
    """LoD build + inverse lifting in one call; the LoD sizes come back in the parameter block"""
    c = pc.case(name)
    lf = pc.lift_params_of(c, npl=[len(c["xyz"])])
    rec = ctx.lift_decode_attr(pc.lod_params_of(c), lf, c["xyz"], c["coeffs"], lcp=c["lcp"],
                               min_geom_node_size_log2=c["m"], geom_num_points=c["N"])
    pc.assert_attrs(rec, c, name)
    assert list(lf.num_points_in_lod[:lf.num_lods]) == list(c["npl"])


def test_whole_slice_weights_would_not_decode_it(ctx):
    """the fixture tells the two weight rules apart: the whole-slice entry over the same predictors differs
    (a case with N > P: with N = P both rules give the finest level weight 1 and the coarser ones N / size)"""
    c = pc.case("tiny_m2")
    assert c["N"] > len(c["xyz"])
    lod = c["lod"]
    rec = ctx.lift_inverse(pc.lift_params_of(c), lod["nc"], lod["ni"], lod["w"], lod["indexes"], c["coeffs"], lcp=c["lcp"])
    assert not np.array_equal(rec, c["attrs"])


def test_dev_lift_decode_attr_partial_ragged_batch(ctx):
    """three cases of the fixture as one batch resident in HBM, each with its own full point count"""
    import torch
    dev = torch.device("cuda:0")
    cases = [pc.case(n) for n in pc.BATCH]
    assert len({(c["m"], c["max_neigh_range"]) for c in cases}) == 1
    sizes = [len(c["xyz"]) for c in cases]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offsets[-1])
    d_xyz = torch.from_numpy(np.concatenate([c["xyz"] for c in cases])).to(dev)
    d_co = torch.from_numpy(np.concatenate([c["coeffs"] for c in cases]).reshape(-1)).to(dev)
    d_dec = torch.zeros(3 * n, dtype=torch.int32, device=dev)
    d_indexes = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lfs = [pc.lift_params_of(c, npl=[s]) for c, s in zip(cases, sizes)]
    lcp = np.stack([c["lcp"] for c in cases])
    ctx.dev_lift_attr(False, pc.lod_params_of(cases[0]), lfs, offsets, d_xyz.data_ptr(), d_dec.data_ptr(), d_co.data_ptr(),
                      3, lcp=lcp, d_indexes=d_indexes.data_ptr(), min_geom_node_size_log2=cases[0]["m"],
                      geom_num_points=[c["N"] for c in cases])
    dec, indexes = d_dec.cpu().numpy().reshape(-1, 3), d_indexes.cpu().numpy()
    lp = pc.lod_params_of(cases[0])
    for i, c in enumerate(cases):
        a, b = int(offsets[i]), int(offsets[i + 1])
        pc.assert_attrs(dec[a:b], c, pc.BATCH[i])
        lod = ctx.lod_build(lp, c["xyz"], min_geom_node_size_log2=c["m"], geom_num_points=c["N"])
        pc.assert_lod(lod, c, pc.BATCH[i])
        np.testing.assert_array_equal(indexes[a:b], lod["indexes"], err_msg=pc.BATCH[i])
        assert list(lfs[i].num_points_in_lod[:lfs[i].num_lods]) == list(c["npl"])


def test_first_level_zero_is_the_existing_entries(ctx):
    """m = 0, N = P through the new entries = the existing entries, on a 200 k cloud"""
    from mpeg_pcc_tmc13_amd import lift_params, synth
    xyz, attrs = synth.dense_cloud(200_000, seed=61, bits=10)
    n = len(xyz)
    lp = pc.lod_params_of(dict(max_neigh_range=5))
    want = ctx.lod_build(lp, xyz)
    got = ctx.lod_build(lp, xyz, min_geom_node_size_log2=0, geom_num_points=n)
    for k in pc.LOD_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    lf = lift_params([n], qp=31, scalable=True)
    co, rec, lcp, _ = ctx.lift_encode_attr(lp, lf, xyz, attrs)
    lf = lift_params(want["npl"], qp=31, scalable=True)
    a = ctx.lift_inverse(lf, want["nc"], want["ni"], want["w"], want["indexes"], co, lcp=lcp)
    b = ctx.lift_inverse(lf, want["nc"], want["ni"], want["w"], want["indexes"], co, lcp=lcp,
                         min_geom_node_size_log2=0, geom_num_points=n)
    np.testing.assert_array_equal(a, rec)
    np.testing.assert_array_equal(b, rec)
    d = ctx.lift_decode_attr(lp, lift_params([n], qp=31), xyz, co, lcp=lcp, min_geom_node_size_log2=0, geom_num_points=n)
    np.testing.assert_array_equal(d, rec)


def test_partial_decode_at_full_size_is_self_consistent(ctx):
    """a 1 M-point dense cloud decoded at m = 2: the one-call entry = LoD build + inverse lifting over its
    result (no reference fixture of this size is committed)"""
    from mpeg_pcc_tmc13_amd import lift_params, synth
    xyz = synth.dense_cloud(1_000_000, seed=62, bits=11)[0]
    N, m = len(xyz), 2
    order = np.argsort(synth.morton_codes(xyz), kind="stable")
    q = (xyz[order] >> m) << m
    _, first = np.unique(q, axis=0, return_index=True)
    part = np.ascontiguousarray(q[np.sort(first)] + (1 << (m - 1)), dtype=np.int32)
    P = len(part)
    assert N // 8 < P < N
    rng = np.random.default_rng(62)
    coeffs = (rng.integers(-40, 41, size=(P, 3)) * (rng.random((P, 3)) < 0.2)).astype(np.int32)
    lcp = rng.integers(-2, 3, size=32).astype(np.int8)
    lp = pc.lod_params_of(dict(max_neigh_range=5))
    lod = ctx.lod_build(lp, part, min_geom_node_size_log2=m, geom_num_points=N)
    assert lod["npl"][-1] == P and len(lod["npl"]) <= 21 - m
    assert sorted(lod["indexes"]) == list(range(P))
    lf = lift_params(lod["npl"], qp=34, scalable=True)
    want = ctx.lift_inverse(lf, lod["nc"], lod["ni"], lod["w"], lod["indexes"], coeffs, lcp=lcp,
                            min_geom_node_size_log2=m, geom_num_points=N)
    lf1 = lift_params([P], qp=34)
    got = ctx.lift_decode_attr(lp, lf1, part, coeffs, lcp=lcp, min_geom_node_size_log2=m, geom_num_points=N)
    np.testing.assert_array_equal(got, want)
    assert list(lf1.num_points_in_lod[:lf1.num_lods]) == list(lod["npl"])


def test_partial_decode_declines(ctx):
    """what stays off the device says so: the predicting transform, and arguments that make no slice"""
    from mpeg_pcc_tmc13_amd import _lib
    c = pc.case("dense_m2_small")
    lp = pc.lod_params_of(c)
    lp.attr_encoding = 1
    with pytest.raises(_lib.GpccError, match="predicting transform"):
        ctx.lod_build(lp, c["xyz"], min_geom_node_size_log2=c["m"], geom_num_points=c["N"])
    lp = pc.lod_params_of(c)
    with pytest.raises(_lib.GpccError, match="geom_num_points"):
        ctx.lod_build(lp, c["xyz"], min_geom_node_size_log2=c["m"], geom_num_points=len(c["xyz"]) - 1)
    with pytest.raises(_lib.GpccError, match="min_geom_node_size_log2"):
        ctx.lod_build(lp, c["xyz"], min_geom_node_size_log2=21, geom_num_points=c["N"])
