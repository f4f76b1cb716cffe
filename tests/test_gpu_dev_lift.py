"""The lifting transform of the device tier over a held LoD structure on the MI355X: gpcc_dev_lod_build once, then
gpcc_dev_lift_forward / gpcc_dev_lift_inverse per attribute, a batch of slices per call (csrc/lift_batch.hpp).

Expected, slice by slice: the host tier's own gpcc_lift_forward / gpcc_lift_inverse on that slice's downloaded
structure; the C oracle (dev_lift_cases); gpcc_dev_lift_encode_attr / _decode_attr called for an attribute alone; the
same slice between other neighbours; and the bookkeeping of the launches, the pool and the check kernel's refusal.
Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import dev_lift_cases as lc
from mpeg_pcc_tmc13_amd import lod_params
from mpeg_pcc_tmc13_amd.params import lift_params_of_lod

pytestmark = pytest.mark.gpu
SENTINEL = -77


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    assert hasattr(c, "dev_lift")
    yield c
    c.close()


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


class Structure:
    """a batch's LoD structure in HBM"""

    def __init__(self, count, index, weight, indexes, npl):
        self.count, self.index, self.weight, self.indexes, self.npl = count, index, weight, indexes, npl

    def ptrs(self):
        return self.count.data_ptr(), self.index.data_ptr(), self.weight.data_ptr(), self.indexes.data_ptr()

    def host(self):
        n = self.count.numel()
        return (self.count.cpu().numpy(), self.index.cpu().numpy().reshape(n, 3), self.weight.cpu().numpy().reshape(n, 3),
                self.indexes.cpu().numpy())


def build(ctx, lp, offsets, xyz):
    """gpcc_dev_lod_build -> Structure"""
    import torch
    n = int(offsets[-1])
    d_xyz = to_dev(xyz)
    st = Structure(filled(n), filled(3 * n), filled(3 * n), filled(n), None)
    torch.cuda.synchronize()
    st.npl = [[int(v) for v in row] for row in ctx.dev_lod_build(lp, offsets, d_xyz.data_ptr(), *st.ptrs())]
    ctx.synchronize()
    return st


def upload(structure, npl):
    return Structure(*(to_dev(a) for a in structure), npl)


def forward(ctx, params, offsets, st, attrs, c, xyz=None):
    """-> (coeffs [N, c], reconstruction [N, c], lcp [S, 32]); the structure must come back unchanged"""
    import torch
    n = int(offsets[-1])
    d_a, d_c = to_dev(attrs), filled(n * c)
    d_xyz = None if xyz is None else to_dev(xyz)
    before = st.host()
    torch.cuda.synchronize()
    lcp = ctx.dev_lift(True, params, offsets, *st.ptrs(), d_a.data_ptr(), d_c.data_ptr(), c,
                       d_xyz=None if xyz is None else d_xyz.data_ptr())
    for got, want in zip(st.host(), before):
        np.testing.assert_array_equal(got, want)
    return d_c.cpu().numpy().reshape(n, c), d_a.cpu().numpy().reshape(n, c), lcp


def inverse(ctx, params, offsets, st, coeffs, lcp, c, xyz=None):
    """-> the reconstruction [N, c], decoded into sentinel-filled attributes"""
    import torch
    n = int(offsets[-1])
    d_c, d_a = to_dev(coeffs), filled(n * c)
    d_xyz = None if xyz is None else to_dev(xyz)
    torch.cuda.synchronize()
    ctx.dev_lift(False, params, offsets, *st.ptrs(), d_a.data_ptr(), d_c.data_ptr(), c, lcp=lcp,
                 d_xyz=None if xyz is None else d_xyz.data_ptr())
    np.testing.assert_array_equal(d_c.cpu().numpy(), np.asarray(coeffs).reshape(-1))
    return d_a.cpu().numpy().reshape(n, c)


# ---- 1. build, then forward and inverse: the host tier and the oracle ---------------------------------------------
def parity(ctx, name, c, lcp, bitdepth, mode="plain"):
    b = lc.batch(name)
    st = build(ctx, lc.lod_params_of(name), b.offsets, b.xyz)
    assert st.npl == b.npl
    params = b.params(c, lcp, bitdepth, mode, npl=st.npl)
    attrs = b.attrs(c, bitdepth)
    xyz = b.xyz if mode == "regions" else None
    co, rec, l = forward(ctx, params, b.offsets, st, attrs, c, xyz)
    dec = inverse(ctx, params, b.offsets, st, co, l, c, xyz)
    np.testing.assert_array_equal(dec, rec, err_msg="the inverse's output is not the forward's reconstruction")
    nc, ni, nw, ix = st.host()
    exp = lc.expected(name, c, lcp, bitdepth, mode)
    assert co.any()
    for s in range(len(b.lengths)):
        what = f"{name} c={c} lcp={lcp} {bitdepth} bit {mode}: slice {s} ({b.lengths[s]} points, LoDs {b.npl[s]})"
        q = b.region_offsets(s, mode)
        sl = [b.slice(a, s) for a in (nc, ni, nw, ix)]
        h_co, h_rec, h_lcp = ctx.lift_forward(params[s], *sl, b.slice(attrs, s), qp_off=q)
        h_dec = ctx.lift_inverse(params[s], *sl, h_co, lcp=h_lcp, qp_off=q)
        for which, (w_co, w_rec, w_lcp, w_dec) in (("host tier", (h_co, h_rec, h_lcp, h_dec)),
                                                    ("oracle", (exp[s][0], exp[s][1], exp[s][2], exp[s][1]))):
            np.testing.assert_array_equal(b.slice(co, s), w_co, err_msg=f"{what}: coefficients, {which}")
            np.testing.assert_array_equal(b.slice(rec, s), w_rec, err_msg=f"{what}: reconstruction, {which}")
            np.testing.assert_array_equal(b.slice(dec, s), w_dec, err_msg=f"{what}: decoded, {which}")
            if c == 3 and lcp:
                np.testing.assert_array_equal(l[s], w_lcp, err_msg=f"{what}: LCP coefficients, {which}")


@pytest.mark.parametrize("c,lcp,bitdepth", [(3, True, 8), (1, False, 16), (3, False, 16)])
def test_distance_batch_equals_the_host_tier_and_the_oracle(ctx, c, lcp, bitdepth):
    parity(ctx, "distance", c, lcp, bitdepth)


def test_ragged_batch_equals_the_host_tier_and_the_oracle(ctx):
    parity(ctx, "ragged", 3, True, 8)


def test_scalable_weights_equal_the_host_tier_and_the_oracle(ctx):
    parity(ctx, "distance", 3, True, 8, "scalable")


# ---- 2. two attributes over one build -----------------------------------------------------------------------------
def test_two_attributes_over_one_build_equal_the_coder_called_for_each_alone(ctx):
    import torch
    b = lc.batch("distance")
    lp = lod_params()
    n = int(b.offsets[-1])
    st = build(ctx, lp, b.offsets, b.xyz)
    refl = (np.random.default_rng(12).integers(0, 1024, (n, 1))).astype(np.int32)
    for c, attrs, kw in ((3, b.attrs(3, 8), dict(qp=31, bitdepth=8, lcp=True)),
                         (1, refl, dict(qp=43, chroma_offset=0, bitdepth=10, lcp=False))):
        params = [lift_params_of_lod(row, **kw) for row in st.npl]
        co, rec, l = forward(ctx, params, b.offsets, st, attrs, c)
        dec = inverse(ctx, params, b.offsets, st, co, l, c)
        # the parent's way: the coder builds the structure itself, per attribute
        alone = [lift_params_of_lod([1], **kw) for _ in st.npl]
        d_xyz, d_a, d_c, d_ix = to_dev(b.xyz), to_dev(attrs), filled(n * c), filled(n)
        torch.cuda.synchronize()
        w_l = ctx.dev_lift_attr(True, lp, alone, b.offsets, d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), c,
                                d_indexes=d_ix.data_ptr())
        ctx.synchronize()
        w_co, w_rec = d_c.cpu().numpy().reshape(n, c), d_a.cpu().numpy().reshape(n, c)
        d_dec = filled(n * c)
        torch.cuda.synchronize()
        ctx.dev_lift_attr(False, lp, alone, b.offsets, d_xyz.data_ptr(), d_dec.data_ptr(), d_c.data_ptr(), c, lcp=w_l)
        ctx.synchronize()
        assert [list(p.num_points_in_lod[:p.num_lods]) for p in alone] == st.npl
        np.testing.assert_array_equal(d_ix.cpu().numpy(), st.indexes.cpu().numpy())
        np.testing.assert_array_equal(co, w_co, err_msg=f"c={c}: coefficients")
        np.testing.assert_array_equal(rec, w_rec, err_msg=f"c={c}: reconstruction")
        np.testing.assert_array_equal(dec, d_dec.cpu().numpy().reshape(n, c), err_msg=f"c={c}: decoded")
        np.testing.assert_array_equal(l, w_l, err_msg=f"c={c}: LCP coefficients")
        assert co.any() and (c == 1 or l.any())


# ---- 3. neighbour independence ------------------------------------------------------------------------------------
def test_a_slice_does_not_depend_on_its_neighbours(ctx):
    b = lc.batch("distance")
    c, lcp, bitdepth = 3, True, 8
    params, attrs = b.params(c, lcp, bitdepth, "regions"), b.attrs(c, bitdepth)
    mid = b.lengths.index(257)   # the slice with the overlapping boxes

    def run(before, after):
        pick = before + [mid] + after
        offsets = np.concatenate([[0], np.cumsum([b.lengths[s] for s in pick])]).astype(np.int64)
        st = upload([np.concatenate([np.asarray(b.lods[s][k]).astype(np.int32) for s in pick]) for k in ("nc", "ni", "w", "indexes")],
                    [b.npl[s] for s in pick])
        xyz = np.concatenate([b.slice(b.xyz, s) for s in pick])
        p = [params[s] for s in pick]
        co, rec, l = forward(ctx, p, offsets, st, np.concatenate([b.slice(attrs, s) for s in pick]), c, xyz)
        dec = inverse(ctx, p, offsets, st, co, l, c, xyz)
        k = len(before)
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        return co[lo:hi], rec[lo:hi], l[k], dec[lo:hi]

    i = b.lengths.index
    alone = run([], [])
    for before, after in (([i(64), i(4097)], [i(255)]), ([i(255)], [i(1), i(65)]), ([i(1)] * 3, []), ([], [i(4097)])):
        for a, g, what in zip(alone, run(before, after), ("coefficients", "reconstruction", "LCP", "decoded")):
            np.testing.assert_array_equal(g, a, err_msg=f"{what} between {before} and {after}")
    assert alone[0].any() and alone[2].any()


# ---- 4. regions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,lcp,bitdepth", [(3, True, 8), (1, False, 16)])
def test_region_offsets_formed_on_the_spot_equal_the_host_tier_given_the_array(ctx, c, lcp, bitdepth):
    b = lc.batch("distance")
    parity(ctx, "distance", c, lcp, bitdepth, "regions")
    boxes = [lc.boxes_of("distance", s, n) for s, n in enumerate(b.lengths)]
    assert any(len(r) == 8 for r in boxes) and any(len(r) == 0 for r in boxes) and any(len(r) == 2 for r in boxes)
    # points ON each of the six faces of the faces box, inside it and outside it
    s = b.lengths.index(255)
    (lo, hi, _), = boxes[s]
    xyz = b.slice(b.xyz, s)
    inside = np.all((xyz >= lo) & (xyz <= hi), axis=1)
    assert (~inside).any()
    for k in range(3):
        assert (inside & (xyz[:, k] == lo[k])).any() and (inside & (xyz[:, k] == hi[k])).any(), k
    # points in the corner two overlapping boxes share take the FIRST box's offset
    s = b.lengths.index(257)
    (lo0, hi0, off0), (lo1, hi1, off1) = boxes[s]
    xyz = b.slice(b.xyz, s)
    both = np.all((xyz >= lo1) & (xyz <= hi0), axis=1)
    assert both.any() and off0 != off1 and (b.region_offsets(s, "regions")[both] == off0).all()


# ---- 5. the launches ----------------------------------------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_number_of_slices(ctx):
    """the periodic batch as 3 and as 300 slices of the same total: the same number of launches"""
    total, c, lcp, bitdepth = 19200, 3, True, 8   # slices of 6400 and of 64 points: no LoD is empty in either batch
    counts, levels = {}, {}
    for slices in (3, 300):
        b = lc.Batch("periodic", [total // slices] * slices, seed=900)
        st = build(ctx, lc.lod_params_of("periodic"), b.offsets, b.xyz)
        assert st.npl == b.npl
        levels[slices] = max(len(v) for v in st.npl)
        params = b.params(c, lcp, bitdepth, npl=st.npl)
        ctx.set_profiling(True)
        try:
            ctx.kernel_times()
            co, rec, l = forward(ctx, params, b.offsets, st, b.attrs(c, bitdepth), c)
            inverse(ctx, params, b.offsets, st, co, l, c)
            counts[slices] = {k: v[1] for k, v in ctx.kernel_times().items()}
        finally:
            ctx.set_profiling(False)
        print(slices, "slices:", sum(counts[slices].values()), "launches", counts[slices])
    assert levels[3] == levels[300] == 4
    assert counts[3] == counts[300]
    assert sum(counts[3].values()) <= (7 + 7 * 3) + (5 + 4 * 3)
    assert counts[3]["lift_batch_check"] == 2 and counts[3]["lift_batch_quantise"] == 2


# ---- 6. the pool --------------------------------------------------------------------------------------------------
def test_a_second_call_of_the_shape_allocates_nothing(ctx):
    b = lc.batch("distance")
    c, lcp, bitdepth = 3, True, 8
    st = upload(b.structure(), b.npl)
    params, attrs = b.params(c, lcp, bitdepth), b.attrs(c, bitdepth)
    in_use = debug_words(ctx, "gpcc_debug_pool_in_use", 2)
    results = []
    for k in range(2):
        events = debug_words(ctx, "gpcc_debug_alloc_events", 4)
        co, rec, l = forward(ctx, params, b.offsets, st, attrs, c)
        dec = inverse(ctx, params, b.offsets, st, co, l, c)
        if k == 1:
            assert debug_words(ctx, "gpcc_debug_alloc_events", 4) == events   # no pool miss, no arena growth
        assert debug_words(ctx, "gpcc_debug_pool_in_use", 2) == in_use
        results.append((co, rec, l, dec))
    for f, s in zip(*results):
        np.testing.assert_array_equal(f, s)


def test_a_refusal_leaves_the_pool_whole_and_the_buffers_untouched(ctx):
    import torch
    from mpeg_pcc_tmc13_amd._lib import GpccError
    b = lc.batch("distance")
    c = 3
    n = int(b.offsets[-1])
    st = upload(b.structure(), b.npl)
    good = b.params(c, True, 8)
    d_a, d_c = filled(n * c), filled(n * c)
    torch.cuda.synchronize()
    in_use = debug_words(ctx, "gpcc_debug_pool_in_use", 2)

    def spoilt(**fields):
        p = b.params(c, True, 8)
        for k, v in fields.items():
            setattr(p[-1], k, v)
        return p
    with_region = b.params(c, True, 8, "regions")
    for fwd in (True, False):
        for params, kw in ((spoilt(bitdepth=17), {}), (spoilt(num_qp_regions=9), {}), (spoilt(num_lods=0), {}),
                           (with_region, {}), (good, dict(c=4)), (good, dict(offsets=[0, n]))):
            with pytest.raises(GpccError) as e:
                ctx.dev_lift(fwd, params if "offsets" not in kw else params[:1], kw.get("offsets", b.offsets), *st.ptrs(),
                             d_a.data_ptr(), d_c.data_ptr(), kw.get("c", c))
            assert e.value.code == -1
            assert debug_words(ctx, "gpcc_debug_pool_in_use", 2) == in_use
    ctx.synchronize()
    assert (d_a.cpu().numpy() == SENTINEL).all() and (d_c.cpu().numpy() == SENTINEL).all()


# ---- 7. the check kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fwd", [True, False])
def test_a_neighbour_in_its_predictors_own_level_is_refused_by_the_check_kernel(ctx, fwd):
    """the index is in bounds whether or not the guard works: no GPU test feeds an out-of-range index (those kinds
    are tested under the emulator)"""
    import torch
    from mpeg_pcc_tmc13_amd._lib import GpccError
    b = lc.batch("distance")
    c = 3
    n = int(b.offsets[-1])
    nc, ni, nw, ix = (a.copy() for a in b.structure())
    s = b.lengths.index(65)
    base, npl = int(b.offsets[s]), b.npl[s]
    i = npl[2] + 1
    assert nc[base + i] >= 1 and npl[2] < i < npl[3]
    ni[base + i, 0] = npl[2]
    assert 0 <= ni[base + i, 0] < b.lengths[s]
    st = upload((nc, ni, nw, ix), b.npl)
    params = b.params(c, True, 8)
    d_a, d_c = filled(n * c), filled(n * c)
    lcp = np.full((len(b.lengths), 32), 0x5A, np.int8)
    torch.cuda.synchronize()
    in_use = debug_words(ctx, "gpcc_debug_pool_in_use", 2)
    offs = np.ascontiguousarray(b.offsets, dtype=np.int64)
    from mpeg_pcc_tmc13_amd.params import LiftParams
    arr = (LiftParams * len(params))(*params)
    fn = ctx._lib.gpcc_dev_lift_forward if fwd else ctx._lib.gpcc_dev_lift_inverse
    rc = fn(ctx._h, arr, len(params), offs.ctypes.data_as(C.POINTER(C.c_int64)), *st.ptrs(), None, d_a.data_ptr(),
            d_c.data_ptr(), lcp.ctypes.data, c)
    assert rc == -1 and b"coarser level" in ctx._lib.gpcc_last_error()
    ctx.synchronize()
    assert (d_a.cpu().numpy() == SENTINEL).all() and (d_c.cpu().numpy() == SENTINEL).all() and (lcp == 0x5A).all()
    assert debug_words(ctx, "gpcc_debug_pool_in_use", 2) == in_use
    # the context serves the next valid call
    good = upload(b.structure(), b.npl)
    co, rec, _ = forward(ctx, params, b.offsets, good, b.attrs(c, 8), c)
    np.testing.assert_array_equal(co, np.concatenate([e[0] for e in lc.expected("distance", c, True, 8)]))
    with pytest.raises(GpccError):
        ctx.dev_lift(fwd, params, b.offsets, *st.ptrs(), d_a.data_ptr(), d_c.data_ptr(), c)
