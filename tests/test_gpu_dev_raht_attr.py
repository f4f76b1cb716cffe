"""The RAHT slice coder of the device tier on the MI355X: gpcc_dev_raht_encode_attr / gpcc_dev_raht_decode_attr, a
batch of slices in HBM from point order in one call (Morton sort, gather with the region QP offsets, transform, clip,
scatter).

Expected, slice by slice: the host tier's own call for that slice alone (gpcc_raht_encode_attr,
gpcc_raht_encode_attr_packed_regions, gpcc_raht_decode_attr_regions, gpcc_attr_morton_sort); the C oracle
(oracle_attr_morton_sort -> raht_forward with raht_cases._qp_region offsets -> clip -> scatter) and, where it is built,
the compiled reference's transform; the same slice between other neighbours; three chains that stay in HBM; and the
bookkeeping of the pool, the refusals and the launches.  Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import dev_raht_attr_cases as dc
import lod_helpers as lh
import oracle_loader as ol
import symbol_stream_cases as sc
from mpeg_pcc_tmc13_amd import raht_params
from mpeg_pcc_tmc13_amd.params import qp_regions

pytestmark = pytest.mark.gpu
SENTINEL = -77
FLAGS = {
    "default": (),
    "compact": (("subnode", False),),                              # the compact level pass
    "haar": (("qp", 4), ("haar", True), ("chroma_offset", 0)),     # integer Haar, lossless
}
CB = [(1, 10), (3, 8), (3, 16)]
RAGGED = [(3, 8, "default", "mixed"), (1, 10, "compact", "none")]   # the 300-slice batch runs in two configurations


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    assert hasattr(c, "dev_raht_attr")
    yield c
    c.close()


def params_of(bitdepth, flags):
    kw = dict(flags)
    return raht_params(bitdepth=bitdepth, **kw) if "qp" in kw else dc.params_of(bitdepth, **kw)


def to_dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).reshape(-1).copy()).to("cuda:0")


def filled(words, value=SENTINEL):
    import torch
    return torch.full((max(int(words), 1),), value, dtype=torch.int32, device="cuda:0")


def debug_words(ctx, name, n):
    from mpeg_pcc_tmc13_amd import _lib
    fn = getattr(_lib.load(), name)
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * n)()
    assert fn(ctx._h, out) == 0
    return list(out)


def structs(regions):
    return None if regions is None else [qp_regions(r) for r in regions]


def dev_encode(ctx, p, offsets, xyz, attrs, c, bitdepth, regions=None, order=True):
    """-> (coeffs flat, clipped reconstruction [N, c] point order, order [N] or None)"""
    import torch
    n = int(offsets[-1])
    d_xyz, d_a = to_dev(xyz), to_dev(attrs)
    d_c, d_o = filled(n * c), filled(n)
    torch.cuda.synchronize()
    ctx.dev_raht_attr(True, p, offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c, bitdepth, structs(regions),
                      d_o.data_ptr() if order else None)
    ctx.synchronize()
    np.testing.assert_array_equal(d_xyz.cpu().numpy(), np.asarray(xyz).reshape(-1))
    if not order:
        assert (d_o.cpu().numpy() == SENTINEL).all()
    return d_c.cpu().numpy(), d_a.cpu().numpy().reshape(n, c), d_o.cpu().numpy() if order else None


def dev_decode(ctx, p, offsets, xyz, coeffs, c, bitdepth, regions=None):
    """-> the clipped reconstruction [N, c] in point order, decoded into sentinel-filled attributes"""
    import torch
    n = int(offsets[-1])
    d_xyz, d_c = to_dev(xyz), to_dev(coeffs)
    d_a = filled(n * c)
    torch.cuda.synchronize()
    ctx.dev_raht_attr(False, p, offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c, bitdepth, structs(regions))
    ctx.synchronize()
    np.testing.assert_array_equal(d_c.cpu().numpy(), coeffs)
    return d_a.cpu().numpy().reshape(n, c)


_dev = {}


def dev_results(ctx, name, c, bitdepth, mode, flags):
    """the batch of the table through both entries, once per key: (coeffs, encoder's attrs, order, decoder's attrs)"""
    key = (name, c, bitdepth, mode, flags)
    if key not in _dev:
        b = dc.batch(name, c, bitdepth)
        p = params_of(bitdepth, FLAGS[flags])
        regions = dc.regions_of(name, mode)
        co, rec, order = dev_encode(ctx, p, b.offsets, b.xyz, b.attrs, c, bitdepth, regions)
        dec = dev_decode(ctx, p, b.offsets, b.xyz, co, c, bitdepth, regions)
        _dev[key] = (co, rec, order, dec)
    return _dev[key]


def planar_of_symbols(runs, values, trailing, n, c):
    logical = sc.stream_of_symbols(runs, values, trailing) if len(runs) else np.zeros((n, c), np.int32)
    assert logical.shape == (n, c)
    return np.ascontiguousarray(logical.T).reshape(-1)


def host_tier(ctx, p, xyz, attrs, boxes, bitdepth):
    """the host tier's own calls for one slice -> (coeffs planar, encoder's attrs, order, decoder's attrs)"""
    n, c = attrs.shape
    if boxes:
        r = qp_regions(boxes)
        runs, values, trailing, rec = ctx.raht_encode_attr_packed_regions(p, r, xyz, attrs, bitdepth)
        co = planar_of_symbols(runs, values, trailing, n, c)
    else:
        r = None
        co, rec = ctx.raht_encode_attr(p, xyz, attrs, bitdepth)
    dec = ctx.raht_decode_attr_regions(p, r, xyz, co, c, bitdepth)
    return co, rec, ctx.morton_sort(xyz)[1], dec


def check_slices(b, got, want_of, what):
    co, rec, order, dec = got
    for s in range(len(b.lengths)):
        lo, hi = int(b.offsets[s]), int(b.offsets[s + 1])
        w_co, w_rec, w_order, w_dec = want_of(s)
        np.testing.assert_array_equal(co[b.c * lo:b.c * hi], w_co, err_msg=f"{what}: coefficients of slice {s}")
        np.testing.assert_array_equal(rec[lo:hi], w_rec, err_msg=f"{what}: encoder's reconstruction of slice {s}")
        np.testing.assert_array_equal(order[lo:hi], w_order, err_msg=f"{what}: order of slice {s}")
        np.testing.assert_array_equal(dec[lo:hi], w_dec, err_msg=f"{what}: decoder's reconstruction of slice {s}")


# ---- 1. host-tier parity ------------------------------------------------------------------------------------------
def host_parity(ctx, name, c, bitdepth, mode, flags):
    b = dc.batch(name, c, bitdepth)
    p = params_of(bitdepth, FLAGS[flags])
    regions = dc.regions_of(name, mode)
    got = dev_results(ctx, name, c, bitdepth, mode, flags)
    assert got[0].any()

    def want(s):
        return host_tier(ctx, p, b.slice(b.xyz, s), b.slice(b.attrs, s), regions[s] if regions else [], bitdepth)
    check_slices(b, got, want, (name, c, bitdepth, mode, flags))


@pytest.mark.parametrize("mode", dc.REGION_MODES)
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("c,bitdepth", CB)
def test_edge_batch_equals_the_host_tier_slice_by_slice(ctx, c, bitdepth, flags, mode):
    host_parity(ctx, "edges", c, bitdepth, mode, flags)


@pytest.mark.parametrize("c,bitdepth,flags,mode", RAGGED)
def test_ragged_batch_equals_the_host_tier_slice_by_slice(ctx, c, bitdepth, flags, mode):
    host_parity(ctx, "ragged", c, bitdepth, mode, flags)


# ---- 2. oracle parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c,bitdepth,flags,mode", [("edges", c, bd, f, m) for c, bd in CB for f in FLAGS for m in dc.REGION_MODES]
                         + [("ragged",) + r for r in RAGGED])
def test_batch_equals_the_oracle_and_the_reference(ctx, name, c, bitdepth, flags, mode):
    b = dc.batch(name, c, bitdepth)
    got = dev_results(ctx, name, c, bitdepth, mode, flags)
    for which in ("oracle",) + (("ref",) if ol.ref_available() else ()):
        exp = dc.expected(name, c, bitdepth, mode, FLAGS[flags], which)
        # (the decoder reproduces the encoder's clipped reconstruction)
        check_slices(b, got, lambda s: (exp[s][0], exp[s][1], b.order[s], exp[s][1]), (which, name, c, bitdepth, mode, flags))


# ---- 3. neighbour independence ------------------------------------------------------------------------------------
def test_a_slice_does_not_depend_on_its_neighbours(ctx):
    c, bitdepth = 3, 8
    b = dc.batch("edges", c, bitdepth)
    regions = dc.regions_of("edges", "mixed")
    p = params_of(bitdepth, ())
    mid = dc.LENGTHS.index(255)   # the slice with the faces box

    def run(before, after):
        pick = before + [mid] + after
        offsets = np.concatenate([[0], np.cumsum([b.lengths[s] for s in pick])]).astype(np.int64)
        xyz = np.concatenate([b.slice(b.xyz, s) for s in pick])
        attrs = np.concatenate([b.slice(b.attrs, s) for s in pick])
        reg = [regions[s] for s in pick]
        co, rec, order = dev_encode(ctx, p, offsets, xyz, attrs, c, bitdepth, reg)
        dec = dev_decode(ctx, p, offsets, xyz, co, c, bitdepth, reg)
        k = len(before)
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        return co[c * lo:c * hi], rec[lo:hi], order[lo:hi], dec[lo:hi]

    i = dc.LENGTHS.index
    alone = run([], [])
    for before, after in (([i(64), i(4097)], [i(256)]), ([i(256)], [i(1), i(65)]), ([i(1)] * 3, []), ([], [i(4096)])):
        for a, g, what in zip(alone, run(before, after), ("coefficients", "reconstruction", "order", "decoded")):
            np.testing.assert_array_equal(g, a, err_msg=f"{what} between {before} and {after}")
    assert alone[0].any()


# ---- 4. chains that stay in HBM -----------------------------------------------------------------------------------
def test_spherical_positions_to_bins_without_leaving_the_device(ctx):
    """gpcc_dev_attr_to_spherical -> encode -> gpcc_dev_residual_bins: the bins of the host-tier pair per slice"""
    import torch
    import spherical_cases as sph
    case = sph.case("ragged300")
    offsets = case["offsets"]
    n = int(offsets[-1])
    refl = np.random.default_rng(5).integers(0, 256, (n, 1)).astype(np.int32)
    p = raht_params(qp=34)
    d_xyz, d_a, d_c = to_dev(case["xyz"]), to_dev(refl), filled(n)
    torch.cuda.synchronize()
    ctx.dev_attr_to_spherical(sph.params(case), offsets, d_xyz.data_ptr(), d_xyz.data_ptr())
    ctx.dev_raht_attr(True, p, offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), 1)
    bo, nsym, trail = ctx.dev_residual_bins(offsets, d_c.data_ptr(), 1, True)
    d_bins = torch.zeros(max(int(bo[-1]), 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    bo, nsym, trail = ctx.dev_residual_bins(offsets, d_c.data_ptr(), 1, True, d_bins.data_ptr(), int(bo[-1]))
    ctx.synchronize()
    bins, rec = d_bins.cpu().numpy(), d_a.cpu().numpy().reshape(n, 1)
    assert bo[-1] > 0
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        pos, _ = ctx.attr_to_spherical(sph.params(case), case["xyz"][lo:hi])
        runs, values, trailing, w_rec = ctx.raht_encode_attr_packed(p, pos, refl[lo:hi])
        want = ctx.binarise_symbols(runs, values, trailing, 1)
        np.testing.assert_array_equal(bins[bo[s]:bo[s + 1]], want, err_msg=f"bins of slice {s}")
        np.testing.assert_array_equal(rec[lo:hi], w_rec, err_msg=f"reconstruction of slice {s}")


def test_host_symbols_to_the_decoded_attributes(ctx):
    """host symbols -> gpcc_dev_zero_run_unpack -> decode: the encoder's clipped reconstruction"""
    import torch
    c, bitdepth = 3, 8
    b = dc.batch("edges", c, bitdepth)
    exp = dc.expected("edges", c, bitdepth)
    symbols = []
    for s, n in enumerate(b.lengths):
        logical = np.ascontiguousarray(exp[s][0].reshape(c, n).T)
        runs, values, _ = lh.oracle_zero_run_pack(logical, n, c, False)
        symbols.append((runs, values))
    so = np.concatenate([[0], np.cumsum([len(r) for r, _ in symbols])]).astype(np.int64)
    runs = np.concatenate([np.asarray(r, np.int32) for r, _ in symbols])
    values = np.concatenate([np.asarray(v, np.int32).reshape(-1) for _, v in symbols])
    n = int(b.offsets[-1])
    d_xyz, d_c, d_a = to_dev(b.xyz), filled(n * c), filled(n * c)
    torch.cuda.synchronize()
    ctx.dev_zero_run_unpack(b.offsets, so, runs, values, d_c.data_ptr(), c, True)
    ctx.dev_raht_attr(False, dc.params_of(bitdepth), b.offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c, bitdepth)
    ctx.synchronize()
    np.testing.assert_array_equal(d_c.cpu().numpy(), np.concatenate([e[0] for e in exp]))
    np.testing.assert_array_equal(d_a.cpu().numpy().reshape(n, c), np.concatenate([e[1] for e in exp]))


def test_recoloured_colours_to_coefficients(ctx):
    """gpcc_dev_recolour_attrs -> encode: the coefficients of the route through gpcc_dev_attr_morton_sort, a torch
    gather and gpcc_dev_raht_forward (the chain test of tests/test_gpu_dev_recolour.py)"""
    import torch
    import recolour_batch_cases as rbc
    from mpeg_pcc_tmc13_amd import recolour_params
    dev = torch.device("cuda:0")
    rb = rbc.batch("dense", (2500, 300, 1800), 0.5)
    offsets = rb.tgt_off
    nt = int(offsets[-1])
    sizes = [int(v) for v in np.diff(offsets)]
    d_sx, d_tx = torch.from_numpy(np.array(rb.src_xyz)).to(dev), torch.from_numpy(np.array(rb.tgt_xyz)).to(dev)
    d_src = torch.from_numpy(np.array(rb.attrs[0][0])).to(dev)
    d_out = torch.full((nt, 3), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.dev_recolour_attrs(recolour_params(bitdepth=8), src_offsets=rb.src_off, d_src_xyz=d_sx.data_ptr(), tgt_offsets=offsets,
                           d_tgt_xyz=d_tx.data_ptr(), attrs=[(d_src.data_ptr(), d_out.data_ptr(), 3, rb.attrs[0][1])],
                           scale=rb.scale, offsets=rb.offsets)
    p = raht_params(qp=30, subnode=False)
    ctx.set_morton_bits(21)
    try:
        # the route of a caller without the entry
        d_m = torch.zeros(nt, dtype=torch.int64, device=dev)
        d_o = torch.zeros(nt, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.dev_attr_morton_sort(offsets, d_tx.data_ptr(), d_m.data_ptr(), d_o.data_ptr())
        ctx.synchronize()
        base = torch.from_numpy(np.array(np.repeat(offsets[:-1], sizes))).to(dev)
        d_sorted = d_out[d_o.long() + base].contiguous()
        d_want = torch.zeros(3 * nt, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.dev_raht_forward(p, offsets, d_m.data_ptr(), d_sorted.data_ptr(), d_want.data_ptr(), 3)
        ctx.synchronize()
        want_rec = torch.empty_like(d_out)
        want_rec[d_o.long() + base] = d_sorted.reshape(nt, 3).clamp(0, 255)
        # the entry: one call on the recoloured colours where they are
        d_c = filled(3 * nt)
        torch.cuda.synchronize()
        ctx.dev_raht_attr(True, p, offsets, d_tx.data_ptr(), d_out.data_ptr(), d_c.data_ptr(), 3, 8)
        ctx.synchronize()
    finally:
        ctx.set_morton_bits(0)
    np.testing.assert_array_equal(d_c.cpu().numpy(), d_want.cpu().numpy())
    np.testing.assert_array_equal(d_out.cpu().numpy(), want_rec.cpu().numpy())
    assert d_want.cpu().numpy().any()


# ---- 5. bookkeeping -----------------------------------------------------------------------------------------------
def test_a_second_call_of_the_shape_allocates_nothing(ctx):
    import torch
    c, bitdepth = 3, 8
    b = dc.batch("edges", c, bitdepth)
    regions = structs(dc.regions_of("edges", "mixed"))
    p = dc.params_of(bitdepth)
    n = int(b.offsets[-1])
    d_xyz = to_dev(b.xyz)
    bufs = [(to_dev(b.attrs), filled(n * c), filled(n)) for _ in range(2)]
    torch.cuda.synchronize()
    in_use = debug_words(ctx, "gpcc_debug_pool_in_use", 2)
    results = []
    for k, (d_a, d_c, d_o) in enumerate(bufs):
        events = debug_words(ctx, "gpcc_debug_alloc_events", 4)
        for encode in (True, False):
            ctx.dev_raht_attr(encode, p, b.offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c, bitdepth, regions,
                              d_o.data_ptr())
        ctx.synchronize()
        if k == 1:
            assert debug_words(ctx, "gpcc_debug_alloc_events", 4) == events   # no pool miss, no arena growth
        assert debug_words(ctx, "gpcc_debug_pool_in_use", 2) == in_use
        results.append([t.cpu().numpy() for t in (d_a, d_c, d_o)])
    for f, s in zip(*results):
        np.testing.assert_array_equal(f, s)


def test_every_refusal_leaves_the_pool_whole_and_the_buffers_untouched(ctx):
    import torch
    from mpeg_pcc_tmc13_amd._lib import GpccError
    c, bitdepth = 3, 8
    offsets = np.array([0, 300, 500], np.int64)
    rng = np.random.default_rng(9)
    d_xyz = to_dev(rng.integers(0, 16, (500, 3)))
    attrs, coeffs = rng.integers(0, 256, 1500).astype(np.int32), rng.integers(-9, 9, 1500).astype(np.int32)
    d_a, d_c = to_dev(attrs), to_dev(coeffs)
    torch.cuda.synchronize()
    good = dict(params=raht_params(), offsets=offsets, d_xyz=d_xyz.data_ptr(), d_attrs=d_a.data_ptr(), d_coeffs=d_c.data_ptr(),
                c=c, bitdepth=bitdepth, regions=None)
    bad_layers = raht_params()
    bad_layers.num_qp_layers = 0
    nine = qp_regions([])
    nine.num_qp_regions = 9
    spoils = [dict(d_xyz=0), dict(d_attrs=0), dict(d_coeffs=0), dict(offsets=[1, 300, 500]), dict(offsets=[0, 300, 300]),
              dict(offsets=[0, 300, 200]), dict(offsets=[0, 300, (1 << 29) + 1]), dict(offsets=[0]), dict(c=0), dict(c=4),
              dict(params=bad_layers), dict(bitdepth=0), dict(bitdepth=17), dict(regions=[qp_regions([]), nine])]
    in_use = debug_words(ctx, "gpcc_debug_pool_in_use", 2)
    for encode in (True, False):
        for spoil in spoils:
            a = dict(good, **spoil)
            with pytest.raises(GpccError) as e:
                ctx.dev_raht_attr(encode, a["params"], a["offsets"], a["d_xyz"], a["d_attrs"], a["d_coeffs"], a["c"],
                                  a["bitdepth"], a["regions"])
            assert e.value.code == -1, spoil
            assert debug_words(ctx, "gpcc_debug_pool_in_use", 2) == in_use, spoil
    ctx.synchronize()
    np.testing.assert_array_equal(d_a.cpu().numpy(), attrs)
    np.testing.assert_array_equal(d_c.cpu().numpy(), coeffs)
    # the context works afterwards
    ctx.dev_raht_attr(True, good["params"], offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c, bitdepth)
    ctx.synchronize()
    assert debug_words(ctx, "gpcc_debug_pool_in_use", 2) == in_use
    assert (d_a.cpu().numpy() != attrs).any()


def test_the_launches_do_not_depend_on_the_number_of_slices(ctx):
    """3 and 300 slices of the same total: the same number of launches (gpcc_ctx_kernel_times, profiling on)"""
    import torch
    c, bitdepth, total = 3, 8, 6000
    rng = np.random.default_rng(77)
    xyz = rng.integers(0, 16, (total, 3)).astype(np.int32)
    attrs = (rng.integers(0, 2, (total, c)) * 255).astype(np.int32)
    p = dc.params_of(bitdepth)
    counts = {}
    ctx.set_morton_bits(12)
    ctx.set_profiling(True)
    try:
        for slices in (3, 300):
            offsets = np.arange(slices + 1, dtype=np.int64) * (total // slices)
            regions = [qp_regions([((2, 2, 2), (9, 9, 9), (2, -2))] if s % 2 else []) for s in range(slices)]
            d_xyz, d_a, d_c = to_dev(xyz), to_dev(attrs), filled(total * c)
            torch.cuda.synchronize()
            ctx.kernel_times()
            for encode in (True, False):
                ctx.dev_raht_attr(encode, p, offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c, bitdepth, regions)
            ctx.synchronize()
            counts[slices] = {k: v[1] for k, v in ctx.kernel_times().items()}
            print(slices, "slices:", sum(counts[slices].values()), "launches", counts[slices])
    finally:
        ctx.set_profiling(False)
        ctx.set_morton_bits(0)
    assert counts[3]["raht_gather"] == 2 and counts[3]["raht_clip_scatter"] == 2
    assert sum(counts[3].values()) == sum(counts[300].values())
    assert counts[3] == counts[300]
