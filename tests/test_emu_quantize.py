"""The kernels of csrc/quantize_positions.hpp -- quantise and key, the plan, the stable sort in one or two rounds,
links and heads, the ordered compaction, and the partition's count / scan / emit -- under the CPU wavefront emulator,
launched by the library's own launch functions (tests/emu/quantize_emu_harness.cpp).  Every comparison is exact
equality, against the golden file where the case is stored and against the restatement of tests/quantize_cases.py;
the harness keeps guard bytes around every output and work array.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on the path)
import quantize_cases as qc

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
T = qc.T
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", EMU_DIR, "-f", "quantize.mk", "libquantize_emu.so"], check=True,
                       stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(EMU_DIR, "libquantize_emu.so"))
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        _lib.quantize_emu.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32]
        _lib.partition_emu.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp, i64, vp, vp]
    return _lib


def emu_quantize(c, mode=None, max1=-1, max2=-1):
    """-> (rc, error word, plan, dst_xyz, idx_to_src, src_dup_next)"""
    mode = c["mode"] if mode is None else mode
    src = c["src"]
    n = len(src)
    params = np.array([mode, *c["offset"], *c["clamp_min"], *c["clamp_max"]], np.int32)
    scales = np.array([c["scale"], c["sample_scale"]], np.float32)
    dst, idx, nxt = np.full((n, 3), -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    plan, err = np.zeros(16, np.int32), np.zeros(1, np.int32)
    rc = emu().quantize_emu(params.ctypes.data, scales.ctypes.data, src.ctypes.data, n, dst.ctypes.data,
                            idx.ctypes.data, nxt.ctypes.data, plan.ctypes.data, err.ctypes.data, max1, max2)
    k = max(rc, 0)
    return rc, int(err[0]), plan, dst[:k], idx[:k], nxt


def emu_partition(src, attrs, idx, nxt, indexes, index_offsets, capacity):
    """-> (rc, error word, out_xyz, out_attrs, out_offsets)"""
    src = np.ascontiguousarray(src, np.int32)
    c = 1 if attrs is None else attrs.shape[1]
    io = np.ascontiguousarray(index_offsets, np.int32)
    ix = np.ascontiguousarray(indexes, np.int32)
    ox, oa = np.zeros((capacity, 3), np.int32), np.zeros((capacity, c), np.int32)
    oo, err = np.full(len(io), -1, np.int64), np.zeros(1, np.int32)
    rc = emu().partition_emu(src.ctypes.data, None if attrs is None else attrs.ctypes.data, len(src), c,
                             idx.ctypes.data, len(idx), nxt.ctypes.data, ix.ctypes.data, io.ctypes.data, len(io) - 1,
                             ox.ctypes.data, oa.ctypes.data, capacity, oo.ctypes.data, err.ctypes.data)
    return rc, int(err[0]), ox, oa, oo


SMALL = [n for n in qc.SIZES if 0 < n <= T + 1]


@pytest.mark.parametrize("pattern", qc.PATTERNS)
def test_edge_matrix(pattern):
    for n in SMALL + [2 * T + 1]:
        name = f"edge/{pattern}/{n}"
        c = qc.case(name)
        rc, err, plan, dst, idx, nxt = emu_quantize(c)
        assert rc > 0 and err == 0, (name, rc, err)
        qc.check_against_golden(name, dst, idx, nxt, "emulator")
        want = qc.expected(c)
        for got, w in zip((dst, idx, nxt), want):
            np.testing.assert_array_equal(got, w, err_msg=name)
        # a 12-bit cloud: one short key, as many passes as its bits need
        assert plan[9] == 0 and plan[10] == (sum(plan[6:9]) + 7) // 8 <= 5 and plan[11] == 0
        if pattern == "identical":
            assert plan[10] == 0 and rc == 1


ARITH_SMALL = [a for a in qc.ARITH if len(qc.case(a)["src"]) <= T + 1 or a == "wide_m1"]


@pytest.mark.parametrize("name", ARITH_SMALL)
def test_arithmetic_width_and_sampling_cases(name):
    c = qc.case(name)
    rc, err, plan, dst, idx, nxt = emu_quantize(c)
    assert rc > 0 and err == 0, (name, rc, err)
    qc.check_against_golden(name, dst, idx, nxt, "emulator")
    if name in ("wide_m1", "wide_m2", "full_int32"):
        assert plan[9] == 1 and plan[11] > 0 and sum(plan[6:9]) > 64, plan  # the two-round sort
    if c["mode"] != 2:  # mode 0: mode 1's positions before merging
        rc0, err0, _, keep, _, _ = emu_quantize(c, mode=0)
        assert rc0 == len(c["src"]) and err0 == 0
        assert str(qc.golden()[f"{name}/keep_sha"]) == qc.digest(keep)


def test_unneeded_passes_return_at_once():
    """the host launches as many passes as its bound allows; the plan decides: more launches, the same result"""
    c = qc.case("edge/rand30/257")
    want = qc.expected(c)
    for max1, max2 in ((8, 4), (7, 0)):
        rc, err, plan, dst, idx, nxt = emu_quantize(c, max1=max1, max2=max2)
        assert rc == len(want[1]) and err == 0
        for got, w in zip((dst, idx, nxt), want):
            np.testing.assert_array_equal(got, w)


def test_domain_error_sets_the_sticky_word():
    c = qc._case(1, 4.0, np.array([[1, 2, 3], [1 << 30, 0, 0], [5, 5, 5]], np.int32))
    assert not qc.in_domain(c)
    rc, err, *_ = emu_quantize(c)
    assert err == 8
    c = qc._case(2, 1.0, np.array([[1, 2, 3], [1 << 30, 0, 0]], np.int32), sample_scale=4.0)
    assert not qc.in_domain(c)
    assert emu_quantize(c)[1] == 8
    # the largest coordinate that is in the domain
    c = qc._case(1, 1.0, np.array([[(1 << 31) - 128, -(1 << 31), 0]], np.int32))
    rc, err, _, dst, idx, nxt = emu_quantize(c)
    assert (rc, err) == (1, 0) and dst.tolist() == [[(1 << 31) - 128, -(1 << 31), 0]]


@pytest.mark.parametrize("name", ["edge/rand30/257", "edge/rand95/4097", "edge/long_group/257", "m2_half"])
def test_partition_lists(name):
    c = qc.case(name)
    src = c["src"]
    _, idx, nxt = qc.expected(c)
    rng = np.random.default_rng(5)
    attrs3 = rng.integers(0, 65536, (len(src), 3)).astype(np.int32)
    for what, ix in qc.index_lists(len(idx)).items():
        want = qc.partition(idx, nxt, ix)
        for attrs in (attrs3, attrs3[:, :1].copy(), None):
            rc, err, ox, oa, oo = emu_partition(src, attrs, idx, nxt, ix, [0, len(ix)], len(want) + 3)
            assert (rc, err) == (0, 0), (name, what, rc, err)
            assert oo.tolist() == [0, len(want)]
            np.testing.assert_array_equal(ox[:len(want)], src[want])
            if attrs is not None:
                np.testing.assert_array_equal(oa[:len(want)], attrs[want])
    assert str(qc.golden()[f"{name}/part_sha"]) == qc.digest(qc.partition(idx, nxt, np.arange(len(idx))).astype(np.int32))


def test_partition_ragged_slices_capacity_and_refusals():
    c = qc.case("edge/rand95/4097")
    src = c["src"]
    _, idx, nxt = qc.expected(c)
    ix, io = qc.ragged_slices(len(idx))
    want, off = qc.partition_slices(idx, nxt, ix, io)
    assert (np.diff(io) == 0).sum() >= 10
    rc, err, ox, _, oo = emu_partition(src, None, idx, nxt, ix, io, len(want))
    assert (rc, err) == (0, 0)
    np.testing.assert_array_equal(oo, off)
    np.testing.assert_array_equal(ox, src[want])
    # one short: refused with the offsets filled and nothing written (the harness checks the buffers)
    rc, err, _, _, oo = emu_partition(src, None, idx, nxt, ix, io, len(want) - 1)
    assert (rc, err) == (1, 0)
    np.testing.assert_array_equal(oo, off)
    # an index outside [0, n_dst), a map entry outside [0, n_src), a list that does not ascend, one that leaves
    bad_ix = ix.copy()
    bad_ix[7] = len(idx)
    assert emu_partition(src, None, idx, nxt, bad_ix, io, len(want))[1] == 9
    bad_ix[7] = -1
    assert emu_partition(src, None, idx, nxt, bad_ix, io, len(want))[1] == 9
    bad_map = idx.copy()
    bad_map[ix[0]] = len(src)
    assert emu_partition(src, None, bad_map, nxt, ix, io, len(want))[1] == 9
    tail = int(np.nonzero(nxt == np.arange(len(nxt)))[0][-1])
    for v in (tail - 1, len(src)):  # a cycle (next[i] < i), a pointer behind the array
        bad_next = nxt.copy()
        bad_next[tail] = v
        every = np.arange(len(idx), dtype=np.int32)
        assert emu_partition(src, None, idx, bad_next, every, [0, len(every)], len(src))[1] == 9
