"""GPU tier of gpcc_quantize_positions and gpcc_src_partition: the edge matrix of tests/quantize_cases.py against the
golden file of the compiled reference (tests/golden/quantize_golden.npz) and against the restatement that
tests/test_quantize_golden.py pins to it.  Exact equality throughout."""
import ctypes as C

import numpy as np
import pytest

import oracle_loader as ol
import quantize_cases as qc
from mpeg_pcc_tmc13_amd import _lib, quantize_params, recolour_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mpeg_pcc_tmc13_amd import context
    c = context(0)
    yield c
    c.close()


def params(c, mode=None):
    return quantize_params(c["mode"] if mode is None else mode, c["scale"], c["offset"], c["clamp_min"], c["clamp_max"],
                           c["sample_scale"])


def run_case(ctx, name):
    c = qc.case(name)
    dst, idx, nxt = ctx.quantize_positions(params(c), c["src"])
    qc.check_against_golden(name, dst, idx, nxt, "device")
    for got, want in zip((dst, idx, nxt), qc.expected(c)):
        np.testing.assert_array_equal(got, want, err_msg=name)
    return c, dst, idx, nxt


@pytest.mark.parametrize("pattern", qc.PATTERNS)
def test_edge_matrix(ctx, pattern):
    """every size around the wavefront, the workgroup, the sort's tile and two tiles + 1"""
    for n in qc.SIZES:
        run_case(ctx, f"edge/{pattern}/{n}")


@pytest.mark.parametrize("name", qc.ARITH)
def test_arithmetic_width_and_sampling_cases(ctx, name):
    c, dst, idx, nxt = run_case(ctx, name)
    if c["mode"] != 2:
        # mode 0 equals mode 1's positions before merging; the map pointers are null
        keep, none_idx, none_next = ctx.quantize_positions(params(c, mode=0), c["src"])
        assert none_idx is None and none_next is None and len(keep) == len(c["src"])
        assert str(qc.golden()[f"{name}/keep_sha"]) == qc.digest(keep)
        np.testing.assert_array_equal(keep[idx], dst)


def test_domain_error_leaves_the_buffers_alone_and_the_context_working(ctx):
    src = np.array([[1, 2, 3], [1 << 30, 0, 0], [5, 5, 5]], np.int32)
    for mode, kw in ((1, {}), (0, {}), (2, dict(sample_scale=2.0))):
        with pytest.raises(_lib.GpccError) as e:
            ctx.quantize_positions(quantize_params(mode, 4.0, **kw), src, fill=0x5A5A5A5A)
        assert e.value.code == -1
        for buf in e.value.buffers:
            assert buf is None or (buf == 0x5A5A5A5A).all()
        run_case(ctx, "edge/rand30/257")  # the next call on the same context succeeds


def test_bad_scales_are_refused_before_any_launch(ctx):
    src = np.array([[1, 2, 3]], np.int32)
    ctx.set_profiling(True)
    ctx.kernel_times()
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        for mode, kw in ((0, {}), (1, {}), (2, {}), (2, dict(sample_scale=scale, scale=1.0))):
            p = quantize_params(mode, kw.pop("scale", scale), **kw)
            with pytest.raises(_lib.GpccError) as e:
                ctx.quantize_positions(p, src, fill=77)
            assert e.value.code == -1
            assert all(b is None or (b == 77).all() for b in e.value.buffers)
    assert ctx.kernel_times() == {}
    ctx.set_profiling(False)


def alloc_events(ctx):
    out = (C.c_longlong * 4)()
    _lib.load().gpcc_debug_alloc_events.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert _lib.load().gpcc_debug_alloc_events(ctx._h, out) == 0
    return list(out)


def test_steady_loop_allocates_nothing(ctx):
    c = qc.case("edge/rand30/8193")
    p = params(c)
    _, idx, nxt = ctx.quantize_positions(p, c["src"])
    every = np.arange(len(idx), dtype=np.int32)
    ctx.src_partition(c["src"], None, idx, nxt, every, capacity=len(c["src"]))
    before = alloc_events(ctx)
    for _ in range(10):
        ctx.quantize_positions(p, c["src"])
        ctx.src_partition(c["src"], None, idx, nxt, every, capacity=len(c["src"]))
    assert alloc_events(ctx) == before


# ---- the partition ---------------------------------------------------------------------------------------------
PART_MAPS = ["edge/rand30/257", "edge/rand95/4097", "edge/long_group/8193", "edge/tile_edge/8193", "m2_half", "wide_m1"]


@pytest.mark.parametrize("name", PART_MAPS)
def test_partition_of_every_golden_map(ctx, name):
    """one slice listing every destination index, a permuted list, a list with repeats; c of 1 and 3, positions only"""
    c = qc.case(name)
    src = c["src"]
    _, idx, nxt = qc.expected(c)
    g = qc.golden()
    rng = np.random.default_rng(11)
    attrs3 = rng.integers(0, 65536, (len(src), 3)).astype(np.int32)
    for what, ix in qc.index_lists(len(idx)).items():
        want = qc.partition(idx, nxt, ix)
        if what == "all":
            assert str(g[f"{name}/part_sha"]) == qc.digest(want.astype(np.int32))
        for attrs in (attrs3, attrs3[:, :1].copy(), None):
            ox, oa, oo = ctx.src_partition(src, attrs, idx, nxt, ix)
            assert oo.tolist() == [0, len(want)], (name, what)
            np.testing.assert_array_equal(ox, src[want])
            if attrs is None:
                assert oa is None
            else:
                np.testing.assert_array_equal(oa, attrs[want])


def test_ragged_slices_in_one_call_with_a_fixed_number_of_launches(ctx):
    c = qc.case("edge/rand95/4097")
    src = c["src"]
    _, idx, nxt = qc.expected(c)
    attrs = np.arange(len(src), dtype=np.int32).reshape(-1, 1)
    ix, io = qc.ragged_slices(len(idx), slices=300)
    assert (np.diff(io) == 0).sum() >= 10
    want, off = qc.partition_slices(idx, nxt, ix, io)
    ctx.set_profiling(True)
    ctx.kernel_times()
    ox, oa, oo = ctx.src_partition(src, attrs, idx, nxt, ix, io, capacity=len(want))
    many = ctx.kernel_times()
    np.testing.assert_array_equal(oo, off)
    np.testing.assert_array_equal(ox, src[want])
    np.testing.assert_array_equal(oa[:, 0], want)
    ctx.src_partition(src, attrs, idx, nxt, ix, capacity=len(want))
    one = ctx.kernel_times()
    ctx.set_profiling(False)
    assert {k: v[1] for k, v in many.items()} == {k: v[1] for k, v in one.items()} and len(one) >= 4


def test_sizing_call_and_capacity_one_short(ctx):
    c = qc.case("edge/rand30/4097")
    src = c["src"]
    _, idx, nxt = qc.expected(c)
    ix, io = qc.ragged_slices(len(idx), slices=7)
    want, off = qc.partition_slices(idx, nxt, ix, io)
    lib = _lib.load()
    oo = np.full(len(io), -1, np.int64)
    args = (src.ctypes.data, None, len(src), 1, idx.ctypes.data, len(idx), nxt.ctypes.data, ix.ctypes.data,
            io.ctypes.data, len(io) - 1)
    assert lib.gpcc_src_partition(ctx._h, *args, None, None, 0, oo.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    np.testing.assert_array_equal(oo, off)
    ox = np.full((len(want), 3), 0x33, np.int32)
    oo[:] = -1
    assert lib.gpcc_src_partition(ctx._h, *args, ox.ctypes.data, None, len(want) - 1,
                                  oo.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    np.testing.assert_array_equal(oo, off)
    assert (ox == 0x33).all()
    assert lib.gpcc_src_partition(ctx._h, *args, ox.ctypes.data, None, len(want),
                                  oo.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    np.testing.assert_array_equal(ox, src[want])


def test_bad_indices_and_maps_are_refused(ctx):
    c = qc.case("edge/rand30/257")
    src = c["src"]
    _, idx, nxt = qc.expected(c)
    every = np.arange(len(idx), dtype=np.int32)

    def refused(m, nx, ix):
        with pytest.raises(_lib.GpccError) as e:
            ctx.src_partition(src, None, m, nx, ix, capacity=4 * len(src))
        assert e.value.code == -1
        ox, _, _ = ctx.src_partition(src, None, idx, nxt, every)  # the context works afterwards
        np.testing.assert_array_equal(ox, src[qc.partition(idx, nxt, every)])

    for v in (len(idx), -1, 1 << 30):
        ix = every.copy()
        ix[5] = v
        refused(idx, nxt, ix)
    for v in (len(src), -1):
        m = idx.copy()
        m[3] = v
        refused(m, nxt, every)
    tail = int(np.nonzero(nxt == np.arange(len(nxt)))[0][-1])
    for v in (tail - 1, 0, len(src), -5):  # cycles (next[i] < i) and pointers outside the array
        nx = nxt.copy()
        nx[tail] = v
        refused(idx, nx, every)


def test_long_chain_of_100000_identical_points(ctx):
    """the long-chain bound: one lane walks the whole cloud"""
    n = 100000
    src = np.repeat(np.array([[7, 8, 9]], np.int32), n, axis=0)
    attrs = np.arange(n, dtype=np.int32).reshape(-1, 1)
    dst, idx, nxt = ctx.quantize_positions(quantize_params(1, 1.0), src)
    assert dst.tolist() == [[7, 8, 9]] and idx.tolist() == [0]
    np.testing.assert_array_equal(nxt, np.minimum(np.arange(n) + 1, n - 1))
    ox, oa, oo = ctx.src_partition(src, attrs, idx, nxt, np.zeros(1, np.int32))
    assert oo.tolist() == [0, n]
    np.testing.assert_array_equal(ox, src)
    np.testing.assert_array_equal(oa[:, 0], np.arange(n))


def test_quantise_partition_recolour_connect(ctx):
    """a 3 000-point surface cloud at scale 0.5: quantize_positions -> src_partition (one slice, all indices) ->
    gpcc_recolour onto the quantised positions, against the golden map -> NumPy partition -> the oracle's recolour"""
    name = "surface_half"
    c = qc.case(name)
    src, colours = qc.surface_cloud()
    np.testing.assert_array_equal(src, c["src"])
    dst, idx, nxt = ctx.quantize_positions(params(c), src)
    qc.check_against_golden(name, dst, idx, nxt, "device")
    every = np.arange(len(idx), dtype=np.int32)
    px, pa, _ = ctx.src_partition(src, colours, idx, nxt, every)
    p = recolour_params(bitdepth=8)
    got = ctx.recolour(p, px, pa, dst, scale=c["scale"])

    want_dst, want_idx, want_next = qc.expected(c)
    qc.check_against_golden(name, want_dst, want_idx, want_next)
    order = qc.partition(want_idx, want_next, every)
    np.testing.assert_array_equal(px, src[order])
    np.testing.assert_array_equal(pa, colours[order])
    np.testing.assert_array_equal(got, ol.oracle().recolour(p, src[order], colours[order], want_dst, scale=c["scale"]))
    if ol.ref_available():
        np.testing.assert_array_equal(got, ol.ref().recolour(p, src[order], colours[order], want_dst, scale=c["scale"]))
