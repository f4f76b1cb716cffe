"""The kernels of csrc/symbol_stream.hpp -- a batch of coefficient streams to (run, values) symbols and binary
decisions, and symbols back to dense coefficients -- under the CPU wavefront emulator, launched by the library's own
launch functions (tests/emu/symbol_stream_emu_harness.cpp), against the C oracle slice by slice.  Every comparison is
exact equality; the harness keeps guard bytes around every output and work array.  No GPU needed."""
import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on the path)
import symbol_stream_cases as sc

T = sc.T
SMALL = [n for n in sc.LENGTHS if n <= T + 1]  # (2T + 1 and 4T + 3: test_longer_slices)
CASES = [(c, mode, planar) for c in (1, 3) for mode in sc.modes(c) for planar in (False, True)]


@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_edge_matrix_symbols_and_bins(pattern):
    """every length of the matrix as a slice of one batch: the tiles of a slice end where the slice ends"""
    for c, mode, planar in CASES:
        slices = [sc.stream(pattern, n, c, mode, shift=i) for i, n in enumerate(SMALL)]
        rc, got = sc.emu_bins(slices, planar)
        assert rc == 0, (pattern, c, mode, planar, rc)
        sc.check_batch(slices, got, (pattern, c, mode, planar))


def test_longer_slices():
    """4T + 3: one run covers three whole tiles without a coded position, the carry is the scanned maximum;
    2T + 1: a slice whose last tile holds one position"""
    for c, planar in ((1, True), (3, False)):
        slices = [sc.stream("empty_tiles", 4 * T + 3, c), sc.stream("last_only", 4 * T + 3, c),
                  sc.stream("rand0.5", 2 * T + 1, c), sc.stream("tile_edge", 2 * T + 1, c)]
        rc, got = sc.emu_bins(slices, planar)
        assert rc == 0
        assert got[0][-1] > 0 and got[1][0] == 2 and got[4][1] == 4 * T + 1 - 5 - 1
        sc.check_batch(slices, got, ("empty_tiles", c, planar))


def test_runs_do_not_cross_slices():
    """slice s ends in zeros, slice s + 1 begins with zeros; one-point slices, zero and coded, in between"""
    def one(n, coded, c):
        out = np.zeros((n, c), np.int32)
        out[coded, 0] = -3
        return out
    for c in (1, 3):
        slices = [one(70, [3], c), one(1, [], c), one(90, [80], c), one(1, [0], c), one(T + 5, [], c), one(T + 5, [T + 1], c)]
        for planar in (False, True):
            rc, (bo, nsym, trail, bins, runs, values) = sc.emu_bins(slices, planar)
            assert rc == 0
            assert list(nsym) == [1, 0, 1, 1, 0, 1] and list(trail) == [66, 1, 9, 0, T + 5, 3]
            assert runs[0] == 3 and runs[71] == 80 and runs[161] == 0 and runs[162 + T + 5] == T + 1
            sc.check_batch(slices, (bo, nsym, trail, bins, runs, values), ("adjacent", c, planar))


@pytest.mark.parametrize("c", [1, 3])
def test_run_and_magnitude_class_edges(c):
    rng = np.random.default_rng(77)
    runs = np.array(sc.RUN_EDGES[:-1] * 4, np.int32)
    mags = np.array([sc.MAG_EDGES[i % len(sc.MAG_EDGES)] for i in range(len(runs) * c)], np.int64).reshape(len(runs), c)
    mags[:, 1:] *= rng.integers(0, 2, (len(runs), c - 1))  # (colour: components other than the first may be zero)
    values = (mags * rng.choice([-1, 1], mags.shape)).astype(np.int32)
    logical = sc.stream_of_symbols(runs, values, 12)
    for planar in (False, True):
        rc, got = sc.emu_bins([logical, logical[::-1].copy()], planar)
        assert rc == 0
        sc.check_batch([logical, logical[::-1].copy()], got, ("class edges", c, planar))


def test_capacity_and_no_symbol_output():
    slices = [sc.stream("rand0.5", 257, 3), sc.stream("alternating", T + 1, 3)]
    rc, want = sc.emu_bins(slices, False)
    assert rc == 0
    total = int(want[0][-1])
    # one short: refused with the host arrays filled and the decisions untouched (the harness checks the buffer)
    rc, got = sc.emu_bins(slices, False, capacity=total - 1)
    assert rc == 1
    for k in range(3):
        np.testing.assert_array_equal(got[k], want[k])
    assert (got[3] == 0xEE).all()
    # without symbol outputs: the same decisions
    rc, got = sc.emu_bins(slices, False, symbols=False)
    assert rc == 0
    sc.check_batch(slices, got, "no symbols", symbols=False)


@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_unpack_inverts_pack(pattern):
    for c, mode, planar in CASES:
        slices = [sc.stream(pattern, n, c, mode, shift=i) for i, n in enumerate(SMALL)]
        symbols = [sc.expected(s)[:2] for s in slices]
        rc, err, flat = sc.emu_unpack([len(s) for s in slices], symbols, c, planar)
        assert rc == 0 and err == 0
        np.testing.assert_array_equal(flat, sc.pack_batch(slices, planar)[1])


def test_unpack_range_errors_leave_the_neighbours_alone():
    n, c = 100, 3
    val = np.array([[5, 0, -1]], np.int32)
    neighbour = (np.array([0], np.int32), np.array([[9, 9, 9]], np.int32))
    for planar in (False, True):
        # a symbol that ends exactly at n - 1 is accepted
        rc, err, flat = sc.emu_unpack([n, 2], [(np.array([n - 1], np.int32), val), neighbour], c, planar)
        assert rc == 0 and err == 0
        first = sc.unpack_batch(flat, [0, n, n + 2], c, planar)
        assert (first[0][n - 1] == val[0]).all() and not first[0][:n - 1].any()
        assert (first[1][0] == 9).all() and not first[1][1].any()
        # one behind it, a negative run, an adversarial sum: not written, the error word set, nothing else touched
        for runs in ([n], [-1], [3, -5], [2**31 - 1, 2**31 - 1]):
            r = np.array(runs, np.int32)
            v = np.repeat(val, len(r), axis=0)
            rc, err, flat = sc.emu_unpack([2, n, 2], [neighbour, (r, v), neighbour], c, planar)
            assert rc == 0 and err == 7, (runs, rc, err)
            parts = sc.unpack_batch(flat, [0, 2, n + 2, n + 4], c, planar)
            for k in (0, 2):
                assert (parts[k][0] == 9).all() and not parts[k][1].any()
            ok = np.zeros((n, c), np.int32)
            if runs[0] == 3:
                ok[3] = val[0]
            np.testing.assert_array_equal(parts[1], ok)


@pytest.mark.parametrize("n", [1, 255, 256, 2047, 2048, 2049, 3 * 2048 + 77])
def test_scan_across_its_blocks(n):
    """the exclusive scan that every pass shares (sums, and running maxima from -1), around the edges of its blocks of
    2 048 entries; 64-bit entries whose total passes 2^60 at the largest size"""
    import ctypes as C
    rng = np.random.default_rng(n)
    b = np.where(rng.random(n) < 0.3, rng.integers(0, 1 << 29, n), -1).astype(np.int32)
    for a in (rng.integers(0, 300_000, n).astype(np.int32), rng.integers(1, 1 << 31, n).astype(np.int64) << 18):
        out_sum, out_max = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        f = sc.emu().symbol_stream_emu_scan
        f.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        assert f(n, a.ctypes.data, int(a.dtype == np.int64), b.ctypes.data, out_sum.ctypes.data, out_max.ctypes.data) == 0
        np.testing.assert_array_equal(out_sum, np.concatenate([[0], np.cumsum(a.astype(np.int64))]))
        np.testing.assert_array_equal(out_max, np.maximum.accumulate(np.concatenate([[-1], b.astype(np.int64)])))
        only_sum = np.zeros(n + 1, np.int64)
        assert f(n, a.ctypes.data, int(a.dtype == np.int64), None, only_sum.ctypes.data, None) == 0
        np.testing.assert_array_equal(only_sum, out_sum)
