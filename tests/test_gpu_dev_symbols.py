"""The entropy front end of the device tier on the MI355X: gpcc_dev_residual_bins (a batch of coefficient streams in
HBM to (run, values) symbols and binary decisions) and gpcc_dev_zero_run_unpack (symbols back to dense coefficients).

Expected: the C oracle (oracle_zero_run_pack, oracle_binarise_symbols) slice by slice, the host tier on the same
streams, and -- where the compiled reference is built -- the arithmetic-coded tail of the reference operator's payload
and the encoder's reconstruction, with nothing but symbols, decisions and offsets passing through the host.
Every comparison is exact equality.

Not exercised: a batch with more than 2^32 decisions (the offsets are 64 bit by construction; such a stream is too
large for a test of seconds)."""
import numpy as np
import pytest

import lod_helpers as lh
import oracle_loader as ol
import symbol_stream_cases as sc

pytestmark = pytest.mark.gpu
needs_entropy = pytest.mark.skipif(not lh.entropy_available(), reason="libtmc3_entropy.so not built")
T = sc.T
CASES = [(c, mode, planar) for c in (1, 3) for mode in sc.modes(c) for planar in (False, True)]


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(-1).copy()).to("cuda:0")


def filled(words, value=-7, dtype=None):
    import torch
    return torch.full((max(int(words), 1),), value, dtype=dtype or torch.int32, device="cuda:0")


def dev_bins(ctx, slices, planar, symbols=True, d_co=None):
    """a sizing call, then the call itself -> (bin_offsets, num_symbols, trailing_run, bins, runs, values)"""
    import torch
    c = slices[0].shape[1]
    offsets, flat = sc.pack_batch(slices, planar)
    n = int(offsets[-1])
    d_co = to_dev(flat) if d_co is None else d_co
    torch.cuda.synchronize()
    sized = ctx.dev_residual_bins(offsets, d_co.data_ptr(), c, planar)
    total = int(sized[0][-1])
    d_bins = filled(total, 0xEE, torch.uint8)
    d_runs, d_values = (filled(n), filled(n * c)) if symbols else (None, None)
    torch.cuda.synchronize()
    got = ctx.dev_residual_bins(offsets, d_co.data_ptr(), c, planar, d_bins.data_ptr(), total,
                                d_runs.data_ptr() if symbols else None, d_values.data_ptr() if symbols else None)
    ctx.synchronize()
    for a, b in zip(sized, got):
        np.testing.assert_array_equal(a, b)
    runs = d_runs.cpu().numpy() if symbols else None
    values = d_values.cpu().numpy().reshape(n, c) if symbols else None
    if symbols:
        # behind a slice's symbols nothing is written
        for s in range(len(slices)):
            assert (runs[offsets[s] + got[1][s]:offsets[s + 1]] == -7).all()
            assert (values[offsets[s] + got[1][s]:offsets[s + 1]] == -7).all()
    return got + (d_bins.cpu().numpy()[:total], runs, values)


def dev_unpack(ctx, lengths, symbols, c, planar, guard=64):
    """-> the batch's coefficients flat; the sentinel-filled words around them are checked"""
    import torch
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    so = np.concatenate([[0], np.cumsum([len(r) for r, _ in symbols])]).astype(np.int64)
    runs = np.concatenate([np.asarray(r, np.int32) for r, _ in symbols] + [np.zeros(0, np.int32)])
    values = np.concatenate([np.asarray(v, np.int32).reshape(-1) for _, v in symbols] + [np.zeros(0, np.int32)])
    words = c * int(offsets[-1])
    d = filled(words + 2 * guard, 0x5A5A5A5A)
    torch.cuda.synchronize()
    ctx.dev_zero_run_unpack(offsets, so, runs, values, d.data_ptr() + 4 * guard, c, planar)
    return d, guard, words


def unpacked(ctx, d, guard, words):
    ctx.synchronize()
    return check_guards(d, guard, words)


def check_guards(d, guard, words):
    h = d.cpu().numpy()
    assert (h[:guard] == 0x5A5A5A5A).all() and (h[guard + words:] == 0x5A5A5A5A).all()
    return h[guard:guard + words]


# ---- the edge matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_edge_matrix_symbols_and_bins(pattern, ctx):
    """every length of the matrix as a slice of one batch, both layouts, c = 1 and colour (mixed and single tuples)"""
    for c, mode, planar in CASES:
        slices = [sc.stream(pattern, n, c, mode, shift=i) for i, n in enumerate(sc.LENGTHS)]
        sc.check_batch(slices, dev_bins(ctx, slices, planar), (pattern, c, mode, planar))


@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_unpack_inverts_pack(pattern, ctx):
    """into sentinel-filled coefficients: every position is written"""
    for c, mode, planar in CASES:
        slices = [sc.stream(pattern, n, c, mode, shift=i) for i, n in enumerate(sc.LENGTHS)]
        symbols = [sc.expected(s)[:2] for s in slices]
        got = unpacked(ctx, *dev_unpack(ctx, [len(s) for s in slices], symbols, c, planar))
        np.testing.assert_array_equal(got, sc.pack_batch(slices, planar)[1], err_msg=str((pattern, c, mode, planar)))


# ---- batches ------------------------------------------------------------------------------------------------------
def ragged(count, c):
    rng = np.random.default_rng(300)
    sizes = list(rng.integers(1, 2 * T + 2, count))
    sizes[:4] = [1, 2 * T + 1, T, 1]
    pats = ["rand0.5", "rand0.001", "alternating", "all_zero", "rand0.999", "last_only", "first_only"]
    # (slice 0: one coded point; slice 3: one zero point)
    return [sc.stream(pats[i % len(pats)] if i else "no_zero", int(n), c, shift=i) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("c,planar", [(1, True), (3, False)])
def test_ragged_batch_of_300_slices_and_launch_counts(c, planar, ctx):
    slices = ragged(300, c)
    got = dev_bins(ctx, slices, planar)
    sc.check_batch(slices, got, ("ragged", c, planar))
    symbols = [sc.expected(s)[:2] for s in slices]
    back = unpacked(ctx, *dev_unpack(ctx, [len(s) for s in slices], symbols, c, planar))
    np.testing.assert_array_equal(back, sc.pack_batch(slices, planar)[1])
    # the number of launches does not depend on the number of slices
    ctx.set_profiling(True)
    try:
        counts = []
        for batch in (slices[:1], slices):
            ctx.kernel_times()
            dev_bins(ctx, batch, planar)
            unpacked(ctx, *dev_unpack(ctx, [len(s) for s in batch], [sc.expected(s)[:2] for s in batch], c, planar))
            times = ctx.kernel_times()
            assert {"sym_tile_summary", "sym_count", "sym_emit", "sym_unpack_scatter"} <= set(times)
            counts.append({k: v[1] for k, v in times.items()})
        assert counts[0] == counts[1]
    finally:
        ctx.set_profiling(False)


@pytest.mark.parametrize("c,planar", [(1, True), (3, False)])
def test_5000_tiny_slices(c, planar, ctx):
    """more tiles than one block of the scans takes, and more slices than the small pinned block holds offsets for"""
    rng = np.random.default_rng(5)
    slices = [sc.stream(("rand0.5", "no_zero", "all_zero", "last_only")[i % 4], int(n), c, shift=i)
              for i, n in enumerate(rng.integers(1, 4, 5000))]
    sc.check_batch(slices, dev_bins(ctx, slices, planar), ("5000 slices", c, planar))
    back = unpacked(ctx, *dev_unpack(ctx, [len(s) for s in slices], [sc.expected(s)[:2] for s in slices], c, planar))
    np.testing.assert_array_equal(back, sc.pack_batch(slices, planar)[1])


def test_a_reserved_context_allocates_nothing():
    """gpcc_ctx_reserve covers the workspace of both directions: no allocation event of the context afterwards"""
    import ctypes as C
    from mpeg_pcc_tmc13_amd import _lib, context

    def events(c):
        out = (C.c_longlong * 4)()
        _lib.load().gpcc_debug_alloc_events.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        assert _lib.load().gpcc_debug_alloc_events(c._h, out) == 0
        return list(out)
    slices = ragged(40, 3)
    ctx = context(0)
    try:
        ctx.reserve(sum(len(s) for s in slices), len(slices), 3)
        before = events(ctx)
        got = dev_bins(ctx, slices, False)
        sc.check_batch(slices, got, "reserved")
        unpacked(ctx, *dev_unpack(ctx, [len(s) for s in slices], [sc.expected(s)[:2] for s in slices], 3, False))
        assert events(ctx) == before
    finally:
        ctx.close()


def test_runs_do_not_cross_slices(ctx):
    """slice s ends in zeros, slice s + 1 begins with zeros; one-point slices, zero and coded, inside the batch"""
    def one(n, coded, c):
        out = np.zeros((n, c), np.int32)
        out[coded, c - 1] = -3
        return out
    for c in (1, 3):
        slices = [one(70, [3], c), one(1, [], c), one(90, [80], c), one(1, [0], c), one(T + 5, [], c), one(T + 5, [T + 1], c)]
        for planar in (False, True):
            got = dev_bins(ctx, slices, planar)
            assert list(got[1]) == [1, 0, 1, 1, 0, 1] and list(got[2]) == [66, 1, 9, 0, T + 5, 3]
            assert got[4][0] == 3 and got[4][71] == 80 and got[4][161] == 0 and got[4][162 + T + 5] == T + 1
            sc.check_batch(slices, got, ("adjacent", c, planar))


# ---- class boundaries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_run_and_magnitude_class_edges(c, ctx):
    """runs 0 1 2 3 4 10 11 12 13 2^20 and magnitudes 1 2 3 4 7 8 2^30 2^31 - 1 through the whole entry"""
    rng = np.random.default_rng(77)
    runs = np.array(sc.RUN_EDGES * 4, np.int32)
    m = len(runs)
    mags = np.array([sc.MAG_EDGES[i % len(sc.MAG_EDGES)] for i in range(m * c)], np.int64).reshape(m, c)
    mags[:, 1:] *= rng.integers(0, 2, (m, c - 1))  # (colour: components other than the first may be zero)
    values = (mags * rng.choice([-1, 1], mags.shape)).astype(np.int32)
    logical = sc.stream_of_symbols(runs, values, 1 << 20)
    er, ev, et, _ = sc.expected(logical)
    assert list(er) == list(runs) and (ev == values).all() and et == 1 << 20
    slices = [logical, logical[::-1].copy()]
    for planar in (False, True):
        sc.check_batch(slices, dev_bins(ctx, slices, planar), ("class edges", c, planar))
        got = unpacked(ctx, *dev_unpack(ctx, [len(s) for s in slices], [sc.expected(s)[:2] for s in slices], c, planar))
        np.testing.assert_array_equal(got, sc.pack_batch(slices, planar)[1])


# ---- the host tier ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,planar", [(1, True), (3, False), (3, True)])
def test_agreement_with_the_host_tier(c, planar, ctx):
    slices = [sc.stream("rand0.5", 4 * T + 3, c), sc.stream("rand0.001", 2 * T + 1, c), sc.stream("all_zero", 257, c)]
    bo, nsym, trail, bins, runs, values = dev_bins(ctx, slices, planar)
    for s, logical in enumerate(slices):
        co = np.ascontiguousarray(logical.T) if planar else logical
        h_runs, h_vals, h_trail = ctx.zero_run_pack(co, len(logical), c, planar)
        want = ctx.binarise_symbols(h_runs, h_vals, h_trail, c)
        np.testing.assert_array_equal(bins[bo[s]:bo[s + 1]], want)
        assert nsym[s] == len(h_runs) and trail[s] == h_trail


# ---- capacity -----------------------------------------------------------------------------------------------------
def test_capacity(ctx):
    import torch
    from mpeg_pcc_tmc13_amd._lib import GpccError
    slices = [sc.stream("rand0.5", 257, 3), sc.stream("alternating", T + 1, 3), sc.stream("all_zero", 5, 3)]
    want = dev_bins(ctx, slices, False)  # (a sizing call that succeeds as described, then the exact capacity)
    sc.check_batch(slices, want, "exact capacity")
    total = int(want[0][-1])
    offsets, flat = sc.pack_batch(slices, False)
    d_co = to_dev(flat)
    d_bins = filled(total + 64, 0xEE, torch.uint8)
    torch.cuda.synchronize()
    # one short: refused, the host arrays filled, the decisions untouched
    with pytest.raises(GpccError) as e:
        ctx.dev_residual_bins(offsets, d_co.data_ptr(), 3, False, d_bins.data_ptr(), total - 1)
    assert e.value.code == -1
    for k, name in enumerate(("bin_offsets", "num_symbols", "trailing_run")):
        np.testing.assert_array_equal(getattr(e.value, name), want[k])
    ctx.synchronize()
    assert (d_bins.cpu().numpy() == 0xEE).all()
    # the sizing call takes the same path: the raw entry says GPCC_ERR_INVALID_ARG with the offsets filled
    import ctypes as C
    from mpeg_pcc_tmc13_amd import _lib
    off = (C.c_int64 * 4)(*offsets)
    bo = np.full(4, -1, np.int64)
    rc = _lib.load().gpcc_dev_residual_bins(ctx._h, 3, off, C.c_void_p(d_co.data_ptr()), 3, 0, None, 0,
                                            bo.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None)
    assert rc == -1
    np.testing.assert_array_equal(bo, want[0])
    # ... and succeeds where there is nothing to write
    zero = to_dev(np.zeros(15, np.int32))
    torch.cuda.synchronize()
    bo, nsym, trail = ctx.dev_residual_bins([0, 5], zero.data_ptr(), 3, False)
    assert list(bo) == [0, len(sc.expected(np.zeros((5, 3), np.int32))[3])] and list(trail) == [5]
    # without the symbol outputs: the same decisions, and nothing behind the exact capacity
    got = dev_bins(ctx, slices, False, symbols=False)
    np.testing.assert_array_equal(got[3], want[3])
    ctx.dev_residual_bins(offsets, d_co.data_ptr(), 3, False, d_bins.data_ptr(), total)
    ctx.synchronize()
    h = d_bins.cpu().numpy()
    np.testing.assert_array_equal(h[:total], want[3])
    assert (h[total:] == 0xEE).all()


# ---- unpack -------------------------------------------------------------------------------------------------------
def test_unpack_range_errors_leave_the_neighbours_alone(ctx):
    from mpeg_pcc_tmc13_amd._lib import GpccError
    n, c = 100, 3
    val = np.array([[5, 0, -1]], np.int32)
    neighbour = (np.array([0], np.int32), np.array([[9, 9, 9]], np.int32))
    nothing = (np.zeros(0, np.int32), np.zeros((0, 3), np.int32))
    for planar in (False, True):
        # a symbol that ends exactly at n - 1 is accepted; a slice with no symbols is all zero
        flat = unpacked(ctx, *dev_unpack(ctx, [n, 2, 7], [(np.array([n - 1], np.int32), val), neighbour, nothing], c, planar))
        parts = sc.unpack_batch(flat, [0, n, n + 2, n + 9], c, planar)
        assert (parts[0][n - 1] == val[0]).all() and not parts[0][:n - 1].any()
        assert (parts[1][0] == 9).all() and not parts[1][1].any() and not parts[2].any()
        # one behind it, a negative run, an adversarial sum: GPCC_ERR_INVALID_ARG at synchronize; such a symbol is not
        # written, the guard words and the neighbouring slices are unchanged, and the context works afterwards
        for runs in ([n], [-1], [3, -5], [2**31 - 1, 2**31 - 1]):
            r = np.array(runs, np.int32)
            d, guard, words = dev_unpack(ctx, [2, n, 2], [neighbour, (r, np.repeat(val, len(r), axis=0)), neighbour], c, planar)
            with pytest.raises(GpccError) as e:
                ctx.synchronize()
            assert e.value.code == -1 and "zero-run unpack" in str(e.value), runs
            parts = sc.unpack_batch(check_guards(d, guard, words), [0, 2, n + 2, n + 4], c, planar)
            for k in (0, 2):
                assert (parts[k][0] == 9).all() and not parts[k][1].any()
            ok = np.zeros((n, c), np.int32)
            if runs[0] == 3:
                ok[3] = val[0]
            np.testing.assert_array_equal(parts[1], ok)
            ctx.synchronize()


# ---- chains -------------------------------------------------------------------------------------------------------
def chain_raht(ctx):
    """one RAHT lidar slice: device forward -> (d_coeffs planar, the reconstruction, what the decoder needs)"""
    import torch
    from mpeg_pcc_tmc13_amd import lod_params, raht_params, synth
    xyz, attrs = synth.lidar_cloud(20_000, seed=9)
    n = len(xyz)
    rp = raht_params(qp=34, chroma_offset=0, search_range=2500)
    payload, rec_enc, _ = lh.ref_operator_roundtrip(lod_params(), 0, rp, 34, 0, 8, 1, xyz, attrs)
    morton, sorted_attrs, order = synth.sort_by_morton(xyz, attrs)
    d_m = torch.from_numpy(morton).to("cuda:0")
    d_a, d_c = to_dev(sorted_attrs), filled(n, 0)
    torch.cuda.synchronize()
    ctx.dev_raht_forward(rp, [0, n], d_m.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), 1)

    def decode(d_coeffs):
        d_out = filled(n, 0)
        torch.cuda.synchronize()
        ctx.dev_raht_inverse(rp, [0, n], d_m.data_ptr(), d_out.data_ptr(), d_coeffs.data_ptr(), 1)
        ctx.synchronize()
        return d_out.cpu().numpy()

    def reference_order(rec):
        out = np.zeros((n, 1), np.int32)
        out[order] = np.clip(rec, 0, 255).reshape(n, 1)
        return out
    return dict(n=n, c=1, planar=True, payload=payload[lh.ref_last_abh_size():], rec_enc=rec_enc, d_coeffs=d_c, d_rec=d_a,
                decode=decode, reference_order=reference_order)


def chain_lift(ctx):
    """one lifting colour slice"""
    import torch
    from mpeg_pcc_tmc13_amd import lift_params, lod_params, raht_params, synth
    xyz, attrs = synth.dense_cloud(20_000, seed=9, bits=8)
    n = len(xyz)
    lp = lod_params()
    payload, rec_enc, _ = lh.ref_operator_roundtrip(lp, 2, raht_params(), 34, 0, 8, True, xyz, attrs)
    d_xyz, d_a, d_c = to_dev(xyz), to_dev(attrs), filled(3 * n, 0)
    torch.cuda.synchronize()
    lfs = [lift_params([n], qp=34, chroma_offset=0, lcp=True, bitdepth=8)]
    lcp = ctx.dev_lift_attr(True, lp, lfs, [0, n], d_xyz.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), 3)

    def decode(d_coeffs):
        d_out = filled(3 * n, 0)
        torch.cuda.synchronize()
        lfs2 = [lift_params([n], qp=34, chroma_offset=0, lcp=True, bitdepth=8)]
        ctx.dev_lift_attr(False, lp, lfs2, [0, n], d_xyz.data_ptr(), d_out.data_ptr(), d_coeffs.data_ptr(), 3, lcp=lcp)
        ctx.synchronize()
        return d_out.cpu().numpy()
    return dict(n=n, c=3, planar=False, payload=payload[lh.ref_last_abh_size():], rec_enc=rec_enc, d_coeffs=d_c, d_rec=d_a,
                decode=decode, reference_order=lambda rec: rec.reshape(n, 3))


@needs_entropy
@pytest.mark.skipif(not (ol.ref_available() and lh.entropy_dec_available()), reason="oracle/_ref not built")
@pytest.mark.parametrize("coder", ["raht", "lift"])
def test_chains_with_the_reference_arithmetic_coder(coder, ctx):
    """encoder: device transform -> gpcc_dev_residual_bins -> the reference's arithmetic coder == the arithmetic-coded
    tail of the reference operator's payload.  decoder: the reference's arithmetic decoder on that payload ->
    gpcc_dev_zero_run_unpack -> device inverse == the encoder's reconstruction.  Only decisions, symbols and offsets
    pass through the host."""
    import torch
    ch = (chain_raht if coder == "raht" else chain_lift)(ctx)
    n, c, planar = ch["n"], ch["c"], ch["planar"]
    sized = ctx.dev_residual_bins([0, n], ch["d_coeffs"].data_ptr(), c, planar)
    total = int(sized[0][-1])
    d_bins = filled(total, 0xEE, torch.uint8)
    torch.cuda.synchronize()
    ctx.dev_residual_bins([0, n], ch["d_coeffs"].data_ptr(), c, planar, d_bins.data_ptr(), total)
    ctx.synchronize()
    assert lh.ref_entropy_encode_bins(d_bins.cpu().numpy(), n) == ch["payload"]
    rec = ch["d_rec"].cpu().numpy()
    np.testing.assert_array_equal(ch["reference_order"](rec), ch["rec_enc"])
    # the decoder's side: the symbols as the arithmetic decoder hands them over
    dense = lh.ref_entropy_decode_symbols(ch["payload"], n, c)
    runs, values, _ = lh.oracle_zero_run_pack(dense, n, c, False)
    assert 0 < len(runs) < n
    d, guard, words = dev_unpack(ctx, [n], [(runs, values)], c, planar)
    d_coeffs = d[guard:guard + words]
    np.testing.assert_array_equal(ch["decode"](d_coeffs), rec)
    np.testing.assert_array_equal(check_guards(d, guard, words), ch["d_coeffs"].cpu().numpy())
