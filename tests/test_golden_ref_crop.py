"""tests/golden/ref_crop_golden.npz (the compiled reference's crop of the previous frame to the current slice's
bounding box) against the numpy restatement of tests/ref_crop_cases.py -- the statement the GPU tests of the inter
coders use to crop a frame -- and the fixture's own promises: which cases keep nothing, which keep more than the
slice has points."""
import numpy as np
import pytest

import ref_crop_cases as rc


@pytest.mark.parametrize("name", rc.NAMES)
def test_numpy_restatement_matches_the_reference(name):
    c = rc.case(name)
    bbox, ro, ox, oa = rc.crop_numpy(c["xyz"], c["offsets"], c["frame_xyz"], c["frame_attrs"])
    rc.check(c, bbox, ro, ox, oa)


def test_the_case_list_is_the_fixtures():
    assert list(rc.golden()["names"]) == rc.NAMES
    for n in rc.SIZES:
        want = dict(all=n, none=0, alternating=(n + 1) // 2, first=1, last=1)
        for p in rc.PATTERNS:
            assert rc.case(f"{p}_{n}_c1")["ref_offsets"].tolist() == [0, want[p]], (p, n)


def test_faces_are_inclusive():
    c = rc.case("faces_c1")
    kept = {tuple(p) for p in c["ref_xyz"]}
    for p in c["frame_xyz"]:
        inside = all(rc.LO <= v <= rc.HI for v in p)
        assert (tuple(p) in kept) == inside, p
    assert len(kept) == 9
    assert rc.case("one_point_c3")["ref_offsets"].tolist() == [0, 2]
    assert (rc.case("one_point_c3")["bbox"][0, :3] == rc.case("one_point_c3")["bbox"][0, 3:]).all()


def test_ragged_and_lidar_promises():
    c = rc.case("ragged300")
    kept, sizes = np.diff(c["ref_offsets"]), np.diff(c["offsets"])
    assert len(sizes) == 300 and sizes.min() >= 1 and sizes.max() <= 60 and len(c["frame_xyz"]) == 5000
    assert (kept == 0).sum() >= 10 and (kept > sizes).sum() >= 10
    c = rc.case("lidar8")
    kept = np.diff(c["ref_offsets"])
    assert len(kept) == 8 and (kept > 0).all() and (kept < len(c["frame_xyz"])).any()
