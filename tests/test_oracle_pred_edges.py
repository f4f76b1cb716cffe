"""CPU-only: the predicting transform at the edges of its arithmetic, on the case table of
tests/pred_edge_cases.py, against the committed record of the compiled reference's operator
(golden/pred_edges_golden.npz: inputs AND outputs, no reference needed): the oracle's encoder and decoder
(oracle/pred_oracle.c), and the device encoder's own source under the CPU wavefront emulator
(tests/emu_pred_repair_loader.py: passes, rate recurrence and ordered walk as the library runs them, per-point QP
offsets included).  Where oracle/_ref is present the live compiled reference must reproduce the record, and the
oracle's symbols through the reference's own entropy coder the recorded payload hash.  Bit-exact.

The `tie_*` cases are near-ties between two direct predictors of equal distortion: they fail, in the oracle and
under the emulator alike, when the colour rate estimate is summed per component instead of in one running sum."""
import hashlib
import subprocess
import sys

import numpy as np
import pytest

import emu_pred_repair_loader as emu
import lod_helpers as lh
import oracle_loader as ol
import pred_edge_cases as pec

needs_ref = pytest.mark.skipif(not (ol.ref_available() and lh.entropy_available() and lh.entropy_dec_available()),
                               reason="compiled reference absent")


@pytest.fixture(scope="module")
def golden():
    return pec.Fixture(pec.GOLDEN)


@pytest.fixture(scope="module")
def cases(golden):
    return pec.fixture_cases(golden)


def with_icp(case):
    return case["c"] == 3 and case["pk"]["icp"]


def test_fixture_holds_the_case_table(golden):
    """every case of the table is stored (none beyond it), with the inputs the table generates"""
    table = pec.cases()
    assert 120 <= len(table) <= 150
    assert {k for k in golden.params if k.startswith("case/")} == {"case/" + c["name"] for c in table}
    assert set(pec.TIES) <= {c["name"] for c in table}
    for case in table:
        np.testing.assert_array_equal(golden[case["field"]], pec.field_attrs(case["geom"], case["kind"], case["c"], case["bd"]),
                                      err_msg=case["name"])
        if case["region"] is not None:
            np.testing.assert_array_equal(golden[f"geom/{case['geom']}/{case['set']}"],
                                          pec.qp_offsets(case, pec.positions(case["geom"])), err_msg=case["name"])
    for geom, want in pec.NPL.items():
        for c in (1, 3):
            npl = golden[f"geom/{geom}/c{c}/npl"].tolist()
            assert len(npl) == want if isinstance(want, int) else npl == want
    assert len(set(golden["geom/r300/c3/npl"][-4:].tolist())) == 1


def test_fixture_hits_its_edges(golden, cases):
    """what the generator asserted when it wrote the file, read back from the file; for the share sums 255 / 256,
    the oracle again: the stored symbols are not those of the same case without the weights"""
    by_name = {c[0]["name"]: c for c in cases}

    def rec_of(name):
        return pec.stored(golden, by_name[name][0])[1]

    for bd in (8, 12, 16):
        top = (1 << bd) - 1
        for s in ("qpmax", "chroma_hi", "region_hi"):        # both clips of the write-back
            rec = rec_of(f"r1500/bin_bd{bd}_c3/{s}")
            assert (rec == 0).any() and (rec == top).any()
        case, pp, lod, attrs, q = by_name[f"r1500/bin_bd{bd}_c3/region_lo"]
        raw0, qp0, raw1, qp1 = pec.effective_qps(pp, lod["indexes"], q)
        assert (raw0 < 4).any() and (raw0 == qp0).any() and (raw1 < 4).any()
        case, pp, lod, attrs, q = by_name[f"r1500/bin_bd{bd}_c3/region_hi"]
        raw0, qp0, raw1, qp1 = pec.effective_qps(pp, lod["indexes"], q)
        assert (raw0 > pp.max_qp).any() and (raw0 == qp0).any() and (raw1 > pp.max_qp).any()
        # the threshold scales with the bit depth; spreads on both sides of it
        case, pp, lod, attrs, q = by_name[f"r1500/thr_bd{bd}_c3/qp4"]
        assert pp.adaptive_prediction_threshold == 64 << (bd - 8)
        spread = pec.neighbour_spread(lod, rec_of(case["name"]))
        assert (spread == pp.adaptive_prediction_threshold).any() and (spread == pp.adaptive_prediction_threshold - 1).any()
        # inter-component coefficients 8 and 0; [0,4,4] then [0,1,1] where every sum is zero
        icp = pec.stored(golden, by_name[f"r1500/icp_bd{bd}_c3/qp34"][0])[2]
        assert 8 in icp[:6, 1] and 0 in icp[:6, 2]
        icp = pec.stored(golden, by_name[f"r1500/const_bd{bd}_c3/qp4"][0])[2]
        assert icp[:6].tolist() == [[0, 4, 4]] + [[0, 1, 1]] * 5
    sums = set()
    for case, pp, lod, attrs, q in cases:
        qnw = case["pk"]["quant_neigh_weight"]
        if any(qnw):
            assert list(pp.quant_neigh_weight) == list(qnw)
            plain = pec.pred_parameters(dict(case, pk=dict(case["pk"], quant_neigh_weight=(0, 0, 0))), lod["npl"])
            without = lh.oracle_pred(True, plain, lod, attrs=attrs, qp_off=q)[0]
            assert not np.array_equal(without, pec.stored(golden, case)[0]), case["name"]
            sums.add(sum(qnw))
    assert {255, 256} <= sums


def test_oracle_encoder_vs_fixture(golden, cases):
    for case, pp, lod, attrs, q in cases:
        want_v, want_rec, want_icp, _ = pec.stored(golden, case)
        values, rec, icp, _ = lh.oracle_pred(True, pp, lod, attrs=attrs, qp_off=q)
        np.testing.assert_array_equal(values, want_v, err_msg=case["name"])
        np.testing.assert_array_equal(rec, want_rec, err_msg=case["name"])
        if with_icp(case):
            np.testing.assert_array_equal(icp, want_icp, err_msg=case["name"])


def test_oracle_decoder_vs_fixture(golden, cases):
    for case, pp, lod, attrs, q in cases:
        want_v, want_rec, want_icp, _ = pec.stored(golden, case)
        rec = lh.oracle_pred(False, pp, lod, values=want_v, icp=want_icp, qp_off=q)[1]
        np.testing.assert_array_equal(rec, want_rec, err_msg=case["name"])


def emulated(c):
    """What runs under the emulator: EVERY three-component case with direct predictors (the ties and the colour
    region cases among them) -- the emulator is the only check of the device's source where there is no GPU -- and
    of the one-component cases those that cost little: the region cases and the two small clouds, apart from one
    slice of 700 points that takes five seconds alone.  A 1 500-point colour slice costs one to three seconds (up
    to 32 whole-slice passes, then the walk)."""
    if not c["pk"]["direct"]:
        return False
    if c["c"] == 3:
        return True
    if c["region"] is not None:
        return True
    return c["geom"] != "r1500" and c["name"] != "l700/bin_bd16_c1/qp34/d3a1+qnw255_0_0"


def group_of(name):
    parts = name.split("/")
    return name if len(parts) == 1 else parts[0] + "/" + parts[1]


EMU_CASES = [c["name"] for c in pec.cases() if emulated(c)]
EMU_GROUPS = sorted({group_of(n) for n in EMU_CASES})


@pytest.mark.parametrize("group", EMU_GROUPS)
def test_emulated_device_encoder_vs_fixture(group, golden, cases):
    mine = [c for c in cases if c[0]["name"] in EMU_CASES and group_of(c[0]["name"]) == group]
    assert mine
    for case, pp, lod, attrs, q in mine:
        want_v, want_rec, want_icp, _ = pec.stored(golden, case)
        values, rec, icp, stats = emu.encode(pp, lod, attrs, qp_off=q)
        np.testing.assert_array_equal(values, want_v, err_msg=case["name"])
        np.testing.assert_array_equal(rec, want_rec, err_msg=case["name"])
        if with_icp(case):
            np.testing.assert_array_equal(icp, want_icp, err_msg=case["name"])


def test_emulated_groups_cover_their_cases():
    """every three-component case with direct predictors, every tie and every region case runs, each once"""
    floor = {c["name"] for c in pec.cases() if c["pk"]["direct"] and (c["c"] == 3 or c["region"] is not None)}
    assert floor | set(pec.TIES) <= set(EMU_CASES)
    assert sorted(n for g in EMU_GROUPS for n in EMU_CASES if group_of(n) == g) == sorted(EMU_CASES)


@needs_ref
def test_live_reference_reproduces_the_fixture(golden, cases, tmp_path):
    """the generator's child process per case (the reference aborts the process when its coder buffer overflows):
    symbols, reconstruction, coefficients, LoD structure and payload hash as stored"""
    import concurrent.futures
    import os
    gen = os.path.join(os.path.dirname(pec.GOLDEN), "make_pred_edges_golden.py")

    def child(i):
        out = str(tmp_path / f"case{i}.npz")
        p = subprocess.run([sys.executable, gen, "--case", cases[i][0]["name"], out], capture_output=True, text=True)
        return p.returncode, p.stderr[-300:], out

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        done = list(pool.map(child, range(len(cases))))
    for (case, pp, lod, attrs, q), (rc, err, out) in zip(cases, done):
        assert rc == 0, (case["name"], err)
        z = np.load(out)
        want_v, want_rec, want_icp, want_sha = pec.stored(golden, case)
        np.testing.assert_array_equal(z["values"], want_v, err_msg=case["name"])
        np.testing.assert_array_equal(z["rec_enc"], want_rec, err_msg=case["name"])
        np.testing.assert_array_equal(z["rec_dec"], want_rec, err_msg=case["name"])
        if with_icp(case):
            np.testing.assert_array_equal(z["icp"], want_icp, err_msg=case["name"])
        assert str(z["sha"]) == want_sha, case["name"]
        for k in ("nc", "ni", "indexes", "npl"):
            np.testing.assert_array_equal(z["lod_" + k], lod[k], err_msg=f"{case['name']} {k}")
        np.testing.assert_array_equal(z["lod_w"].astype(np.int32), lod["w"], err_msg=case["name"])


@needs_ref
def test_oracle_symbols_through_the_reference_coder_give_the_stored_payload(golden, cases):
    """zero-run pack the oracle's values, code them with the reference's own PCCResidualsEncoder: the bytes' hash is
    the one recorded from AttributeEncoder::encode"""
    for case, pp, lod, attrs, q in cases:
        values = lh.oracle_pred(True, pp, lod, attrs=attrs, qp_off=q)[0]
        n, c = values.shape
        runs, vals, trailing = lh.oracle_zero_run_pack(values, n, c, planar=False)
        coded = lh.ref_entropy_encode_symbols(c, n, runs, vals, trailing)
        assert hashlib.sha256(coded).hexdigest() == pec.stored(golden, case)[3], case["name"]
