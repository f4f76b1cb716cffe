"""The NumPy float32 restatement of the quantiser and of the partition walk (tests/quantize_cases.py) equals the
compiled reference on every case of tests/golden/quantize_golden.npz.  This pins what the emulator and GPU tiers
compare against for inputs that are not stored.  No GPU needed; exact equality throughout."""
import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on the path)
import quantize_cases as qc


def test_golden_file_holds_every_case_and_only_integers_and_strings():
    g = qc.golden()
    assert list(g["names"]) == qc.NAMES
    for k in g.files:
        assert g[k].dtype.kind in "iuU", (k, g[k].dtype)
    for name in qc.NAMES:
        full = f"{name}/dst" in g.files
        assert full == (len(qc.case(name)["src"]) <= qc.FULL_MAX), name


@pytest.mark.parametrize("name", qc.NAMES)
def test_restatement_equals_reference(name):
    c = qc.case(name)
    assert qc.in_domain(c)
    dst, idx, nxt = qc.expected(c)
    qc.check_against_golden(name, dst, idx, nxt)
    g = qc.golden()
    part = qc.partition(idx, nxt, np.arange(len(idx))).astype(np.int32)
    assert str(g[f"{name}/part_sha"]) == qc.digest(part)
    if f"{name}/part" in g.files:
        np.testing.assert_array_equal(part, g[f"{name}/part"][:len(part)])
    # every source point is visited exactly once
    np.testing.assert_array_equal(np.sort(part), np.arange(len(c["src"])))
    if c["mode"] != 2:  # quantizePositions: the same positions, duplicates kept
        keep = qc.expected(dict(c, mode=0))[0]
        assert str(g[f"{name}/keep_sha"]) == qc.digest(keep)
        np.testing.assert_array_equal(keep[idx], dst)


def test_sampling_cases_merge_points_that_differ():
    """the goldens hold mode 2 with duplicates: groups whose quantised positions are not all equal"""
    for name in ("m2_half", "m2_quarter", "wide_m2"):
        c = qc.case(name)
        dense = name != "wide_m2"  # (27-bit random coordinates: only equal points share a key)
        key, pos = qc.quantise(c)
        _, idx, nxt = qc.reduce_point_set(key, pos)
        assert len(idx) < len(c["src"])
        second = nxt[idx]
        assert (pos[second] != pos[idx]).any() == dense, name


def test_timed_reference_is_recorded():
    g = qc.golden()
    assert list(g["timed/scales_x1000"]) == [1000, 500, 125] and int(g["timed/points"]) == 1000000
    assert (g["timed/reference_us"] > 0).all() and str(g["timed/machine"])
