"""ref_crop_count_kernel, ref_crop_offsets_kernel and ref_crop_scatter_kernel (csrc/ref_crop.hpp), with the bounding
box kernel and the scan they are launched with, under the CPU wavefront emulator against every case of
tests/golden/ref_crop_golden.npz of at most 4 096 frame points (and the ragged batch), i.e. against the reference's
computeBoundingBox + Box3::contains loop: the 16-byte loads and their scalar edges, the ballots and the ranks inside
a wavefront, the bases across wavefronts, tiles and slices, the capacity rule and the domain's error word."""
import numpy as np
import pytest

import emu_ref_crop_loader as el
import ref_crop_cases as rc

SMALL = [n for n in rc.NAMES if n == "ragged300" or len(rc.inputs(n)["frame_xyz"]) <= rc.FULL_MAX]


def run_emu(c, **kw):
    kw.setdefault("misalign", 1 if c["unaligned"] else 0)
    return el.ref_crop(c["xyz"], c["offsets"], c["frame_xyz"], c["frame_attrs"], **kw)


@pytest.mark.parametrize("name", SMALL)
def test_case_matches_the_reference(name):
    c = rc.case(name)
    code, bbox, ro, ox, oa, err = run_emu(c)
    assert code == 0 and err == 0
    rc.check(c, bbox, ro, ox, oa)


@pytest.mark.parametrize("name", ["alternating_65_c1", "alternating_1025_c3", "last_3073_c1", "faces_c3", "lidar8"])
@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_unaligned_arrays_take_the_scalar_path(name, misalign):
    c = rc.case(name)
    code, bbox, ro, ox, oa, err = run_emu(c, misalign=misalign)
    assert code == 0 and err == 0
    rc.check(c, bbox, ro, ox, oa)


@pytest.mark.parametrize("name", ["alternating_1025_c1", "lidar8", "one_point_c3"])
def test_capacity(name):
    """exactly enough is enough; one less fills the offsets and writes nothing"""
    c = rc.case(name)
    total = int(c["ref_offsets"][-1])
    code, bbox, ro, ox, oa, err = run_emu(c, capacity=total)
    assert code == 0
    rc.check(c, bbox, ro, ox, oa)
    code, bbox, ro, ox, oa, err = run_emu(c, capacity=total - 1)
    assert code == 1 and len(ox) == 0
    np.testing.assert_array_equal(ro, c["ref_offsets"])
    np.testing.assert_array_equal(bbox, c["bbox"])


def test_ragged_batch_equals_its_slices_one_by_one():
    c = rc.case("ragged300")
    _, bbox, ro, ox, oa, _ = run_emu(c)
    off = c["offsets"]
    for s in (0, 1, 19, 20, 150, 298, 299):
        one = dict(c, xyz=c["xyz"][off[s]:off[s + 1]], offsets=np.array([0, off[s + 1] - off[s]], np.int64))
        _, b1, r1, x1, a1, _ = run_emu(one)
        np.testing.assert_array_equal(b1[0], bbox[s])
        assert r1[1] == ro[s + 1] - ro[s]
        np.testing.assert_array_equal(x1, ox[ro[s]:ro[s + 1]])
        np.testing.assert_array_equal(a1, oa[ro[s]:ro[s + 1]])


@pytest.mark.parametrize("where", ["frame", "frame_negative", "slice"])
def test_a_coordinate_outside_the_domain_sets_the_error_word(where):
    c = rc.case("alternating_1025_c1")
    fx, cur = c["frame_xyz"].copy(), c["xyz"].copy()
    if where == "frame":
        fx[1030 % len(fx)] = (5, 1 << 21, 5)       # (in the second tile)
    elif where == "frame_negative":
        fx[3] = (-1, 5, 5)
    else:
        cur[1] = (150, 150, 1 << 21)
    *_, err = el.ref_crop(cur, c["offsets"], fx, c["frame_attrs"])
    assert err == 6
    # ... and 2^21 - 1 is inside the domain
    fx = c["frame_xyz"].copy()
    fx[3] = (0, (1 << 21) - 1, 0)
    *_, err = el.ref_crop(c["xyz"], c["offsets"], fx, c["frame_attrs"])
    assert err == 0
