"""CPU-only: the lifting oracle (oracle/lift_oracle.c) at the edges of the
transform's arithmetic and of its LoD tables, on the case table of
tests/lift_edge_cases.py: against the committed fixture of the compiled
reference (golden/lift_edges_golden.npz: inputs AND outputs, no reference
needed) and, under the `ref` mark, against the live compiled reference.  The
fixture's condition -- every case inside the range in which the reference's
arithmetic is exact -- is checked by a stand-alone program under the
signed-overflow sanitizer (tests/lift_range_check.c), which must also be able
to fail.  Bit-exact."""
import os
import subprocess

import numpy as np
import pytest

import lift_edge_cases as lec
import lod_helpers as lh
import oracle_loader as ol

GOLDEN = lec.GOLDEN

needs_ref = [pytest.mark.ref,
             pytest.mark.skipif(not ol.ref_available(), reason="compiled reference absent")]


def _mark(f):
    for m in needs_ref:
        f = m(f)
    return f


@pytest.fixture(scope="module")
def golden():
    return lec.Fixture(GOLDEN)


all_cases = lec.all_cases


def test_fixture_holds_the_case_table(golden):
    """every case of the table is stored (none beyond it), with the inputs the table generates"""
    cases = all_cases(golden)
    assert set(golden.cases()) == {c[0] for c in cases} and len(cases) == len(golden.cases())
    for geom in lec.GEOM:
        for field, c, bd in lec.fields(geom):
            np.testing.assert_array_equal(golden[f"field/{geom}/{field}"], lec.field_attrs(geom, field))
        np.testing.assert_array_equal(golden[f"geom/{geom}/qp_off"], lec.qp_off(lec.GEOM[geom]["n"]))
    nc, d = lec.weight_rows()
    assert len(nc) == 1864
    np.testing.assert_array_equal(golden["weights/nc_in"], nc)
    np.testing.assert_array_equal(golden["weights/dist2"], d)
    # the synthetic structures are what the table builds over the oracle's computeWeights
    o = ol.oracle()
    for table, npl in lec.TABLES.items():
        s = lec.synth_structure(npl, lambda nc_, d_: lh.compute_weights(o, nc_, d_))
        for k in ("nc", "ni", "w", "indexes", "npl"):
            np.testing.assert_array_equal(golden[f"synth/{table}/{k}"], s[k], err_msg=f"{table} {k}")


def test_fixture_hits_its_edges(golden):
    """what the generator asserted when it wrote the file, read back from the file"""
    from mpeg_pcc_tmc13_amd import lift_params
    nl = len(golden["geom/r1500/npl"])
    assert any(8 in golden[f"case/{g_}/lcp_pos/{s}/lcp"][:nl] for g_ in ("r1500",) for s, *_ in lec.param_sets(8))
    assert any(-8 in golden[f"case/{g_}/lcp_neg/{s}/lcp"][:nl] for g_ in ("r1500",) for s, *_ in lec.param_sets(8))
    for geom in lec.GEOM:
        bd = lec.BINARY_BD[geom]
        rec = golden[f"case/{geom}/bin{bd}_c3/qpmax/rec"]
        assert (rec == 0).any() and (rec == (1 << bd) - 1).any()
    assert golden["field/r1500/band16_c3"].max() > 255 << 6      # values far above 8 bits
    npl = golden["geom/r300/npl"]
    assert len(npl) == 10 and len(set(npl.tolist())) < 10        # empty levels from the reference itself
    lf = lift_params(npl, qp=30, chroma_offset=0, bitdepth=14)
    raw0, qp0, raw1, qp1 = lec.effective_qps(lf, lec.i32(golden["geom/r300/indexes"]), lec.qp_off(300))
    assert (raw0 < 4).any() and (raw0 > lf.max_qp).any() and (raw1 < 4).any() and (raw1 > lf.max_qp).any()


def test_lift_oracle_vs_committed_edge_fixture(golden):
    o = ol.oracle()
    for key, lf, lod, attrs, qp_off in all_cases(golden):
        co, rec, lcp = lh.lift(o, True, lf, lod, attrs, qp_off=qp_off)
        np.testing.assert_array_equal(co, golden[key + "/coeffs"], err_msg=key)
        np.testing.assert_array_equal(rec, golden[key + "/rec"], err_msg=key)
        if attrs.shape[1] == 3:
            np.testing.assert_array_equal(lcp[:lf.num_lods], golden[key + "/lcp"][:lf.num_lods], err_msg=key)


def test_lift_oracle_inverse_from_the_fixture(golden):
    o = ol.oracle()
    for key, lf, lod, attrs, qp_off in all_cases(golden):
        inv = lh.lift(o, False, lf, lod, attrs, coeffs=lec.i32(golden[key + "/coeffs"]), lcp=golden[key + "/lcp"],
                      qp_off=qp_off)[1]
        np.testing.assert_array_equal(inv, golden[key + "/rec"], err_msg=key)


def test_compute_weights_oracle_vs_committed_table(golden):
    nc, w = lh.compute_weights(ol.oracle(), golden["weights/nc_in"], golden["weights/dist2"])
    np.testing.assert_array_equal(nc, golden["weights/nc"])
    np.testing.assert_array_equal(w, golden["weights/w"])
    kept = golden["weights/nc"]
    for k in (1, 2, 3):
        rows = kept == k
        assert rows.any()
        assert (golden["weights/w"][rows, :k].astype(np.int64).sum(axis=1) == 256).all()


@_mark
def test_lift_oracle_vs_live_reference_on_the_edge_cases(golden):
    """keeps fixture and reference honest: the live compiled reference gives the stored results, and its
    AttributeLods::generate the stored structures"""
    from mpeg_pcc_tmc13_amd import lod_params
    o, r = ol.oracle(), ol.ref()
    for geom in lec.GEOM:
        lod = lh.ref_lod_generate(lec.cloud(geom)[0], lod_params())
        for k in ("nc", "ni", "indexes", "npl"):
            np.testing.assert_array_equal(lod[k], golden[f"geom/{geom}/{k}"], err_msg=f"{geom} {k}")
        np.testing.assert_array_equal(lod["w"].astype(np.int32), golden[f"geom/{geom}/w"])
    for key, lf, lod, attrs, qp_off in all_cases(golden):
        co_r, rec_r, lcp_r = lh.lift(r, True, lf, lod, attrs, qp_off=qp_off)
        co_o, rec_o, lcp_o = lh.lift(o, True, lf, lod, attrs, qp_off=qp_off)
        np.testing.assert_array_equal(co_r, golden[key + "/coeffs"], err_msg=key)
        np.testing.assert_array_equal(rec_r, golden[key + "/rec"], err_msg=key)
        np.testing.assert_array_equal(co_o, co_r, err_msg=key)
        np.testing.assert_array_equal(rec_o, rec_r, err_msg=key)
        if attrs.shape[1] == 3:
            np.testing.assert_array_equal(lcp_r[:lf.num_lods], golden[key + "/lcp"][:lf.num_lods], err_msg=key)
            np.testing.assert_array_equal(lcp_o[:lf.num_lods], lcp_r[:lf.num_lods], err_msg=key)
    nc, w = lh.compute_weights(r, golden["weights/nc_in"], golden["weights/dist2"])
    np.testing.assert_array_equal(nc, golden["weights/nc"])
    np.testing.assert_array_equal(w, golden["weights/w"])


def test_range_check_program_passes_the_fixture_and_can_fail(golden, tmp_path):
    """tests/lift_range_check.c (the oracle under -fsanitize=signed-integer-overflow, a stand-alone program):
    exit 0 and the stored result on two fixture cases; abnormal end on full-range 16-bit values, where
    `scaled * iQuantWeight` wraps -- the condition the generator puts on every case can fail"""
    from mpeg_pcc_tmc13_amd import lift_params
    exe = lec.build_range_check(str(tmp_path))
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    cases = {c[0]: c for c in all_cases(golden)}
    for key in ("case/r1500/band16_c3/qp4", "case/r1500/rand14_c3/qpoff"):
        _, lf, lod, attrs, qp_off = cases[key]
        lec.write_case_file(case, lf, lod, attrs, qp_off)
        p = subprocess.run([exe, case, out], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        co, rec, lcp = lec.read_range_output(out, *attrs.shape)
        np.testing.assert_array_equal(co, golden[key + "/coeffs"])
        np.testing.assert_array_equal(rec, golden[key + "/rec"])
        np.testing.assert_array_equal(lcp[:lf.num_lods], golden[key + "/lcp"][:lf.num_lods])
    lod = lec.structure(golden, "geom/r1500")
    full16 = lec.cloud("r1500", 3, 16)[1]
    assert full16.max() >= 1 << 15
    lf = lift_params(lod["npl"], qp=4, chroma_offset=0, bitdepth=16, lcp=True)
    lec.write_case_file(case, lf, lod, full16)
    p = subprocess.run([exe, case], capture_output=True, text=True)
    assert p.returncode != 0
    assert "signed integer overflow" in p.stderr and "lift_oracle.c" in p.stderr
