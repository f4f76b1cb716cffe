"""slice_distortion_kernel and rdo_frame_neighbours_kernel (csrc/slice_rdo.hpp) under the CPU wavefront emulator
against numpy: the 16-byte loads and their scalar tail, the butterfly over the wavefront, the LDS combine and the
one atomic per workgroup, for sizes that are no multiple of 4 / 64 / 256 and for one and two candidates."""
import numpy as np
import pytest

import emu_slice_rdo_loader as el


def numpy_dist(rec, orig):
    return np.abs(rec.astype(np.int64) - orig.astype(np.int64)[None, :]).sum(axis=1)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1027, 4099, 20001])
@pytest.mark.parametrize("num", [1, 2])
def test_distortion_vs_numpy(n, num):
    rng = np.random.default_rng(n * 2 + num)
    orig = rng.integers(0, 1 << 16, n)
    rec = rng.integers(0, 1 << 16, (num, n))
    np.testing.assert_array_equal(el.slice_distortion(rec, orig), numpy_dist(rec, orig))


@pytest.mark.parametrize("grid", [1, 3, 8])
def test_distortion_does_not_depend_on_the_grid(grid):
    """(a grid-stride loop: fewer workgroups than 16-byte loads, and more)"""
    rng = np.random.default_rng(grid)
    n = 5003
    orig = rng.integers(0, 256, n)
    rec = np.clip(orig[None, :] + rng.integers(-9, 10, (2, n)), 0, 255)
    np.testing.assert_array_equal(el.slice_distortion(rec, orig, grid), numpy_dist(rec, orig))


def test_distortion_extremes():
    n = 777
    orig = np.zeros(n, np.int32)
    rec = np.stack([np.full(n, 65535, np.int32), np.zeros(n, np.int32)])
    np.testing.assert_array_equal(el.slice_distortion(rec, orig), [65535 * n, 0])
    # the differences are formed in 64 bits
    big = np.stack([np.full(n, 2**31 - 1, np.int32)])
    np.testing.assert_array_equal(el.slice_distortion(big, np.full(n, -2**31, np.int32)), [(2**32 - 1) * n])


def test_frame_neighbours_are_addressed_behind_the_predictors():
    rng = np.random.default_rng(4)
    n = 1000
    count = rng.integers(0, 4, n)
    ni = rng.integers(0, 500, (n, 3))
    ref = rng.integers(0, 2, (n, 3))
    live = np.arange(3)[None, :] < count[:, None]
    want = np.where(live & (ref != 0), ni + n, ni)
    np.testing.assert_array_equal(el.frame_neighbours(count, ref, ni), want)
