#!/usr/bin/env python3
"""Generate tests/golden/pred_edges_golden.npz from the COMPILED REFERENCE (oracle/_ref) at operator level for the
case table tests/pred_edge_cases.py: the predicting transform at the edges of its arithmetic -- both QP clamps of
both quantisers, both clips of the write-back, the eligibility threshold at every bit depth, the inter-component
coefficients 0, 1 and 8, quant_neigh_weight sums on either side of 256, and near-ties among the direct predictors.

Per case: AttributeEncoder::encode + AttributeDecoder::decode on the slice, the symbols (`values`) read back from the
payload by the reference's own entropy decoder, the reconstruction, the inter-component coefficients of the brick
header, the SHA-256 of the arithmetic-coded payload behind that header.  Every reference call runs in a child process
of its own: the reference's coder buffer holds 6 n + 1024 bytes and the process aborts beyond it ("Aec stream
overflow"); a case that ends so is named, and nothing is written.

Nothing is written either unless, for every case, the reference's own round trip holds (encoder's reconstruction ==
decoder's), the oracle (oracle/pred_oracle.c) equals the reference in symbols, reconstruction, coefficients and
inverse, the payload fits, and the edge the case is named for is hit.  The reference's predicting arithmetic is
64-bit throughout, so this agreement is the range check.

The file holds inputs and recorded outputs only; LoD structures, attribute fields and region offsets are stored once.
Run after `make -C oracle`:   python tests/golden/make_pred_edges_golden.py [output path]"""
import concurrent.futures
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401
import lod_helpers as lh  # noqa: E402
import pred_edge_cases as pec  # noqa: E402

LIMIT = 485139  # the largest fixture committed before this one (raht_golden.npz)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def buffer_size(n):
    """PCCResidualsEncoder::start"""
    return 6 * n + 1024


# ---- the child: one case through the reference ---------------------------------------------------
def run_reference(name, out_path):
    case = next(c for c in pec.cases() if c["name"] == name)
    xyz = pec.positions(case["geom"])
    attrs = pec.field_attrs(case["geom"], case["kind"], case["c"], case["bd"])
    lp = pec.lod_parameters(case["geom"], case["c"])
    lod = lh.ref_lod_generate(xyz, lp)
    pp = pec.pred_parameters(case, lod["npl"])
    pk = case["pk"]
    if case["region"] is not None:
        lo, size = pec.REGION_BOX
        lh.ref_set_qp_region((lo, size, case["region"]))
    payload, rec_enc, rec_dec, icp = lh.ref_pred_roundtrip(lp, pp, pk["threshold"], pk["qp"], pk["chroma_offset"], xyz, attrs)
    abh = lh.ref_last_abh_size()
    values = lh.ref_entropy_decode_symbols(payload[abh:], len(xyz), case["c"])
    np.savez(out_path, values=values, rec_enc=rec_enc, rec_dec=rec_dec, icp=icp, coded=len(payload) - abh,
             sha=np.array(hashlib.sha256(payload[abh:]).hexdigest()),
             **{"lod_" + k: np.asarray(v) for k, v in lod.items()})


def reference(case, tmp):
    """-> the child's arrays, or the text of its failure"""
    out = os.path.join(tmp, case["name"].replace("/", "_").replace("+", "_") + ".npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case["name"], out], capture_output=True,
                       text=True)
    if p.returncode != 0 or not os.path.exists(out):
        return f"exit {p.returncode}: {(p.stderr or p.stdout).strip()[-300:]}"
    z = np.load(out)
    return {k: z[k] for k in z.files}


# ---- the edges -------------------------------------------------------------------------------------
def check_edges(case, pp, lod, attrs, q, values, rec, icp, modes):
    """asserts the edge a case is named for; -> a short text of the counts"""
    name, sname, bd, c, pk = case["name"], case["set"], case["bd"], case["c"], case["pk"]
    top = (1 << bd) - 1
    raw0, qp0, raw1, qp1 = pec.effective_qps(pp, lod["indexes"], q)
    notes = []
    if sname == "qpmax20":
        assert (raw0 > pp.max_qp).all(), name
        notes.append("qp0 above max: all")
    if sname == "chroma_lo" and c == 3:
        assert (raw0 == qp0).all() and (raw1 < 4).all(), name
        notes.append("qp1 below 4: all")
    if sname == "chroma_hi" and c == 3:
        assert (raw0 == qp0).all() and (raw1 > pp.max_qp).all(), name
        notes.append("qp1 above max: all")
    if sname in ("region_lo", "region_hi"):
        inside = int((np.asarray(q)[:, 0] != 0).sum())
        assert 0 < inside < len(q), name
        beyond = (raw0 < 4) if sname == "region_lo" else (raw0 > pp.max_qp)
        beyond1 = (raw1 < 4) if sname == "region_lo" else (raw1 > pp.max_qp)
        assert beyond.sum() == inside and beyond1.sum() == inside, name
        notes.append(f"both quantisers clamped at {inside} points, neither at {len(q) - inside}")
    if case["kind"] == "bin" and sname in ("qpmax", "qpmax20", "chroma_hi", "region_hi") and case["geom"] != "l700":
        assert (rec == 0).any() and (rec == top).any() and (rec != attrs).any(), f"{name}: a write-back clip is not reached"
        notes.append(f"rec == 0: {int((rec == 0).sum())}, == max: {int((rec == top).sum())}")
    chosen = sorted(set(int(m) for m in modes if m >= 0))
    if pk["direct"] == 3 and not pk["avg_disabled"] and case["geom"] == "r1500" and case["kind"] == "rand" and c == 3:
        assert chosen == [0, 1, 2, 3], (name, chosen)    # all four modes
    if case["kind"] == "bin" and pk["direct"] == 3 and sname in {"qp4", "qp6", *pec.TIES} and pk["threshold"] == 64:
        assert chosen[-3:] == [1, 2, 3], (name, chosen)  # (lossless 0 / max: the average never wins)
    if pk["direct"]:
        notes.append(f"modes {chosen}")
    else:
        assert not chosen, name
    if pk["avg_disabled"] and pk["direct"]:
        assert 0 not in chosen, (name, chosen)
    if case["kind"] == "const":
        # (the first predictor has no neighbour: its residual is the value itself)
        assert not chosen and values[0, 0] and not values[1:].any(), name
        if sname == "qp4":
            assert np.array_equal(rec, attrs), name
        if c == 3:
            nl = len(lod["npl"])
            # (a level that repeats its predecessor's size is never closed: the running `lod` counter stalls there)
            npl = lod["npl"].tolist()
            want = [[0, 4, 4]] + [[0, 1, 1] if npl[l] > npl[l - 1] else [0, 0, 0] for l in range(1, nl)]
            assert icp[:nl].tolist() == want, (name, icp[:nl])
            notes.append(f"icp [0,4,4] then [0,1,1], [0,0,0] on {want.count([0, 0, 0])} levels")
    if case["kind"] == "thr" and sname == "qp4" and pk["threshold"] == 64:
        t = pec.threshold_of(bd)
        assert pp.adaptive_prediction_threshold == t
        spread = pec.neighbour_spread(lod, rec)
        at, below = spread == t, spread == t - 1
        assert at.any() and below.any() and (modes[at] >= 0).all() and (modes[below] == -1).all(), name
        notes.append(f"spread T: {int(at.sum())} eligible, T-1: {int(below.sum())} not")
    if pk["threshold"] == 0:
        assert ((modes >= 0) == (np.asarray(lod["nc"]) > 1)).all(), name
    if pk["threshold"] == 255:
        spread = pec.neighbour_spread(lod, rec)
        assert ((modes >= 0) == (spread >= 255 << (bd - 8))).all() and (modes >= 0).any() and \
            ((modes == -1) & (np.asarray(lod["nc"]) > 1)).any(), name
    if case["kind"] == "icp":
        nl = len(lod["npl"])
        if pk["icp"]:
            assert 8 in icp[:nl, 1] and 0 in icp[:nl, 2], (name, icp[:nl])
            notes.append(f"icp second {sorted(set(icp[:nl, 1].tolist()))} third {sorted(set(icp[:nl, 2].tolist()))}")
        else:
            assert not icp.any(), name
    qnw = pk["quant_neigh_weight"]
    if any(qnw):
        # the weights decide something: the same case without them gives other symbols
        plain = pec.pred_parameters(dict(case, pk=dict(pk, quant_neigh_weight=(0, 0, 0))), lod["npl"])
        assert not np.array_equal(lh.oracle_pred(True, plain, lod, attrs=attrs, qp_off=q)[0], values), name
        notes.append(f"share sum {sum(qnw)}: " + ("wide path" if sum(qnw) >= 256 else "packed share word"))
    return "; ".join(notes)


# ---- the parent --------------------------------------------------------------------------------------
def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pred_edges_golden.npz")
    table = pec.cases()
    out = pec.FixtureWriter()
    with tempfile.TemporaryDirectory(prefix="pred_edges_") as tmp:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            results = list(pool.map(lambda c: reference(c, tmp), table))
    failed = [(c["name"], r) for c, r in zip(table, results) if isinstance(r, str)]
    for name, text in failed:
        print("REFERENCE FAILED", name, text)
    assert not failed, f"{len(failed)} cases did not run through the reference"

    inputs = hashlib.sha256()
    lods, seen_icp = {}, set()
    for case, r in zip(table, results):
        name, geom, c = case["name"], case["geom"], case["c"]
        xyz = pec.positions(geom)
        attrs = pec.field_attrs(geom, case["kind"], c, case["bd"])
        lod = dict(nc=r["lod_nc"], ni=r["lod_ni"], w=r["lod_w"].astype(np.int32), indexes=r["lod_indexes"], npl=r["lod_npl"])
        assert (r["lod_w"] < (1 << 31)).all()
        if (geom, c) not in lods:
            lods[geom, c] = lod
            for k in ("nc", "ni", "w", "indexes", "npl"):
                out.add(f"geom/{geom}/c{c}/{k}", lod[k])
            print(f"{geom} c={c} npl {lod['npl'].tolist()}")
            want = pec.NPL[geom]
            assert len(lod["npl"]) == want if isinstance(want, int) else list(lod["npl"]) == want, (geom, lod["npl"])
        for k in lod:
            assert np.array_equal(lod[k], lods[geom, c][k]), (name, k)
        if geom == "r300":
            assert len(set(lod["npl"][-4:].tolist())) == 1     # the last four levels of equal size
        if case["field"] + "/0" not in out.index:
            out.add(case["field"], attrs)
        q = pec.qp_offsets(case, xyz)
        if q is not None and f"geom/{geom}/{case['set']}/0" not in out.index:
            out.add(f"geom/{geom}/{case['set']}", q)
        inputs.update(sha(xyz, attrs, *(lod[k] for k in sorted(lod))).encode())
        pp = pec.pred_parameters(case, lod["npl"])
        # the gates
        assert np.array_equal(r["rec_enc"], r["rec_dec"]), f"{name}: the reference's own round trip"
        coded, room = int(r["coded"]), buffer_size(len(xyz))
        assert coded <= room, f"{name}: payload {coded} > {room}"
        values, rec, icp = r["values"], r["rec_enc"], r["icp"]
        o_values, o_rec, o_icp, modes = lh.oracle_pred(True, pp, lod, attrs=attrs, qp_off=q)
        with_icp = c == 3 and case["pk"]["icp"]
        if with_icp:
            assert np.array_equal(o_icp, icp), f"{name}: oracle coefficients != reference\n{o_icp[:8]}\n{icp[:8]}"
        diff = np.flatnonzero((o_values != values).any(axis=1))
        assert not len(diff), f"{name}: oracle symbols != reference in rows {diff[:8]}: {values[diff[0]]} {o_values[diff[0]]}"
        assert np.array_equal(o_rec, rec), f"{name}: oracle reconstruction != reference"
        inv = lh.oracle_pred(False, pp, lod, values=values, icp=icp, qp_off=q)[1]
        assert np.array_equal(inv, rec), f"{name}: oracle inverse != reference"
        notes = check_edges(case, pp, lod, attrs, q, values, rec, icp if with_icp else np.zeros_like(icp), modes)
        if with_icp:
            seen_icp |= set(icp[:len(lod["npl"]), 1:].reshape(-1).tolist())
        print(f"{name:44s} payload {coded:5d} / {room:5d}  {notes}")
        key = "case/" + name
        out.params[key] = repr(dict(sha=str(r["sha"]), coded=coded))
        out.add(key + "/values", values)
        out.add(key + "/rec", rec, base=case["field"])
        out.add(key + "/icp", icp.astype(np.int32) if with_icp else np.zeros((32, 3), np.int32))
    assert {0, 1, 8} <= seen_icp, seen_icp
    print("inter-component coefficients seen:", sorted(seen_icp))
    out.params["inputs"] = inputs.hexdigest()
    out.save(path, date_time=(2020, 1, 1, 0, 0, 0))   # the same bytes from every run
    size = os.path.getsize(path)
    print("wrote", path, "cases", len(table), "bytes", size)
    assert size <= LIMIT, f"{size} bytes: over the limit of {LIMIT}"


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        run_reference(sys.argv[2], sys.argv[3])
    else:
        main()
