"""The kernels of csrc/raht_marshal.hpp -- the gather of a batch's attributes into Morton order with the region QP
offsets formed on the spot, and the clip and scatter back to point order -- under the CPU wavefront emulator, through
the library's own launch functions (tests/emu/raht_marshal_emu_harness.cpp, guard bytes around every array).  The
check is a NumPy restatement: attrs[base + order], raht_cases._qp_region per box in order, np.clip with the inverse
permutation.  Every comparison is exact equality.  No GPU needed."""
import numpy as np
import pytest

import dev_raht_attr_cases as dc

CONFIGS = [(c, bd) for c in (1, 3) for bd in (8, 10, 16)]


def restated_gather(b, regions):
    base = np.repeat(b.offsets[:-1], b.lengths)
    rows = base + b.order_flat()
    qp = None
    if regions is not None and any(len(r) for r in regions):
        qp = np.concatenate([dc.region_offsets(b.slice(b.xyz, s), regions[s])[b.order[s]] for s in range(len(b.lengths))])
    return rows, b.attrs[rows], qp


@pytest.mark.parametrize("name", dc.BATCHES)
@pytest.mark.parametrize("c,bitdepth", CONFIGS)
def test_gather(name, c, bitdepth):
    b = dc.batch(name, c, bitdepth)
    for mode in dc.REGION_MODES:
        regions = dc.regions_of(name, mode)
        _, want, want_qp = restated_gather(b, regions)
        rcode, got, got_qp = dc.emu_gather(b, regions)
        assert rcode == 0, (mode, rcode)
        np.testing.assert_array_equal(got, want, err_msg=f"{mode}: attributes in Morton order")
        if want_qp is None:
            assert got_qp is None
        else:
            np.testing.assert_array_equal(got_qp, want_qp, err_msg=f"{mode}: region offsets")
            assert (want_qp != 0).any() and (want_qp == 0).all(axis=1).any()


@pytest.mark.parametrize("name", dc.BATCHES)
def test_gather_of_the_decoder_writes_offsets_only(name):
    b = dc.batch(name, 3, 8)
    regions = dc.regions_of(name, "mixed")
    _, _, want_qp = restated_gather(b, regions)
    rcode, got, got_qp = dc.emu_gather(b, regions, attrs=False)
    assert rcode == 0 and got is None
    np.testing.assert_array_equal(got_qp, want_qp)
    # without a region the decoder launches nothing: the harness sees both outputs untouched
    rcode, _, got_qp = dc.emu_gather(b, None, attrs=False)
    assert rcode == 0 and got_qp is None


def test_region_table_has_its_cases():
    b = dc.batch("edges", 3, 8)
    regions = dc.regions_of("edges", "mixed")
    assert dc.check_faces(b, regions) >= 2
    assert any(len(r) == 8 for r in regions) and any(len(r) == 0 for r in regions)
    assert dc.regions_of("edges", "none") is None
    # the overlapping boxes: points in the shared corner take the FIRST box's offset
    s = dc.LENGTHS.index(256)
    (lo0, hi0, off0), (lo1, hi1, off1) = regions[s]
    xyz = b.slice(b.xyz, s)
    both = np.all((xyz >= lo1) & (xyz <= hi0), axis=1)
    assert both.any() and off0 != off1
    assert (dc.region_offsets(xyz, regions[s])[both] == off0).all()


@pytest.mark.parametrize("name", dc.BATCHES)
@pytest.mark.parametrize("c,bitdepth", CONFIGS)
def test_clip_scatter(name, c, bitdepth):
    b = dc.batch(name, c, bitdepth)
    # the oracle's unclipped reconstruction: it leaves [0, 2^bitdepth - 1] on both sides (asserted by the table)
    rec = np.concatenate([e[2] for e in dc.expected(name, c, bitdepth)])
    rows, _, _ = restated_gather(b, None)
    inverse = np.empty_like(rows)
    inverse[rows] = np.arange(len(rows))
    want = np.clip(rec, 0, b.maxv)[inverse]
    rcode, got = dc.emu_clip_scatter(b, rec)
    assert rcode == 0, rcode
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, np.concatenate([e[1] for e in dc.expected(name, c, bitdepth)]))
