"""rpl_convert_kernel and rpl_scale_kernel (csrc/spherical.hpp) under the CPU wavefront emulator against every case
of tests/golden/spherical_golden.npz, i.e. against the reference's convertXyzToRpl + offsetAndScale: the 16-byte
loads and their scalar edges, the tables in LDS, the butterfly and the per-slice atomics of the bounding box, the
ragged batch whose slices must not bleed into each other, the in-place form and the domain's error word."""
import numpy as np
import pytest

import emu_spherical_loader as el
import spherical_cases as sc

UNIT = dict(scale=(256, 256, 256), mode=1, min_pos=(0, 0, 0))  # offsetAndScale as the identity: the unscaled result


def entry_input(c, run):
    """the Cartesian cloud, or -- convert = 0 -- the unscaled result of the case it derives from, taken from `run`
    and pinned to that case's digest"""
    if c["convert"]:
        return c["xyz"]
    base = sc.case(c["of"])
    rpl = run(dict(base, **UNIT))[0]
    assert sc.digest(rpl) == base["rpl_sha"]
    return rpl


def check(c, pos, bbox):
    np.testing.assert_array_equal(bbox, c["bbox"])
    if "pos" in c:
        np.testing.assert_array_equal(pos, c["pos"])
    assert sc.digest(pos) == c["pos_sha"]


def run_emu(c, **kw):
    pos, bbox, err = el.to_spherical(sc.params(c), c["offsets"], c["xyz"], **kw)
    assert err == 0
    return pos, bbox


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_matches_the_reference(name):
    c = sc.case(name)
    c["xyz"] = entry_input(c, run_emu)
    check(c, *run_emu(c))
    if c["convert"] and c["bbox"].max() < (1 << 21):
        # the unscaled (r, phi, laser) as well (all cases but "corners", whose radii a unit scale leaves too large)
        rpl, bbox = run_emu(dict(c, **UNIT))
        np.testing.assert_array_equal(bbox, c["bbox"])
        if "rpl" in c:
            np.testing.assert_array_equal(rpl, c["rpl"])
        assert sc.digest(rpl) == c["rpl_sha"]


@pytest.mark.parametrize("name", ["size_5", "size_257", "hand_synth64", "ragged300", "lidar_2000_s1", "lidar_2000_s1_sph_min2"])
@pytest.mark.parametrize("misalign", [0, 1])
def test_in_place_and_unaligned(name, misalign):
    """pos_out == xyz, and arrays that do not start on a 16-byte boundary (every point takes the scalar path)"""
    c = sc.case(name)
    c["xyz"] = entry_input(c, run_emu)
    check(c, *run_emu(c, in_place=True, misalign=misalign))
    check(c, *run_emu(c, misalign=misalign))


def test_ragged_batch_equals_its_slices_one_by_one():
    c = sc.case("ragged300")
    pos, bbox = run_emu(c)
    off = c["offsets"]
    for s in (0, 1, 17, 150, 298, 299):
        one = dict(c, xyz=c["xyz"][off[s]:off[s + 1]], offsets=np.array([0, off[s + 1] - off[s]], np.int64))
        p1, b1 = run_emu(one)
        np.testing.assert_array_equal(p1, pos[off[s]:off[s + 1]])
        np.testing.assert_array_equal(b1[0], bbox[s])


def test_slices_longer_than_a_tile_in_one_batch():
    """slices of several tiles that start at every alignment, against the same points one slice at a time"""
    c = sc.case("lidar_200000_s1")
    xyz = c["xyz"][:9001]
    off = np.array([0, 1, 1026, 1027, 3078, 5131, 9001], np.int64)
    pos, bbox = run_emu(dict(c, xyz=xyz, offsets=off))
    for s in range(len(off) - 1):
        p1, b1 = run_emu(dict(c, xyz=xyz[off[s]:off[s + 1]], offsets=np.array([0, off[s + 1] - off[s]], np.int64)))
        np.testing.assert_array_equal(p1, pos[off[s]:off[s + 1]])
        np.testing.assert_array_equal(b1[0], bbox[s])


@pytest.mark.parametrize("bad", [(1 << 22, 0, 0), (0, -(1 << 22), 0), (0, 0, 1 << 22), (2**31 - 1, 0, 0), (0, -2**31, 5)])
def test_a_point_outside_the_domain_sets_the_error_word(bad):
    c = sc.case("size_65")
    xyz = c["xyz"].copy()
    xyz[40] = np.clip(np.array(bad, np.int64) + c["origin"], -2**31, 2**31 - 1)
    _, _, err = el.to_spherical(sc.params(c), c["offsets"], xyz)
    assert err == 5
    # ... and a scaled coordinate outside [0, 2^21): a minimum above the smallest value, a scale too large
    for change in (dict(mode=1, min_pos=(c["bbox"][0][0] + 1, 0, 0)), dict(scale=(256 * 16, 256, 256))):
        _, _, err = el.to_spherical(sc.params(dict(c, **change)), c["offsets"], c["xyz"])
        assert err == 5, change


def test_iatan2_and_find_laser_on_their_own():
    lib = el.lib()
    # the octants' edges (misc.cpp:297-309): 0, pi/4, pi/2, pi in 20-bit fixed point
    assert lib.spherical_emu_iatan2(0, 0) == 0
    assert lib.spherical_emu_iatan2(0, 1000) == 0 and lib.spherical_emu_iatan2(0, -1000) == 3294199
    assert lib.spherical_emu_iatan2(1000, 0) == 1647099 and lib.spherical_emu_iatan2(-1000, 0) == -1647099
    assert abs(lib.spherical_emu_iatan2(1000, 1000) - 823549) <= 256
    assert lib.spherical_emu_iatan2(-7, -9) == -(3294199 - lib.spherical_emu_iatan2(7, 9))
    # the tie rule and the ends of the table (geometry_octree.cpp:866-871); rinv = 2^14: theta32 == z
    t3 = np.array([-10, 0, 11], np.int32)
    want = {-100: 0, -10: 0, -6: 0, -5: 0, -4: 1, 0: 1, 5: 1, 6: 2, 11: 2, 100: 2}
    for z, laser in want.items():
        assert lib.spherical_emu_find_laser(z, 1 << 14, t3, 3) == laser, z
    t2 = np.array([-10, 10], np.int32)
    assert [lib.spherical_emu_find_laser(z, 1 << 14, t2, 2) for z in (-50, 0, 1, 50)] == [0, 0, 1, 1]
    assert lib.spherical_emu_find_laser(12345, 1 << 14, t2, 1) == 0
