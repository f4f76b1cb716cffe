#!/usr/bin/env python3
"""Generate tests/golden/lift_edges_golden.npz from the COMPILED REFERENCE
(oracle/_ref/libtmc3_ref.so) for the case table tests/lift_edge_cases.py: the
lifting transform at the edges of its arithmetic (value range, both QP clamps,
both clips of the last-component coefficient, both clips of the write-back) and
of its LoD tables (empty levels, more QP layers than levels), and
PCCPredictor::computeWeights on a table of squared-distance triples.

Every lifting case is run through tests/lift_range_check.c first (the oracle
under the signed-overflow sanitizer, a stand-alone program): the reference's
arithmetic wraps once a coefficient reaches about 2^15 attribute units, and a
wrapped case has no defined result.  The generator refuses to write when one
case fails that check, when the oracle and the reference differ anywhere, or
when an edge a case is there for is not hit.

The file holds inputs and recorded outputs only; LoD structures, attribute
fields and the distance table are stored once."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401
import lift_edge_cases as lec  # noqa: E402
import lod_helpers as lh  # noqa: E402
import oracle_loader as ol  # noqa: E402
from mpeg_pcc_tmc13_amd import lift_params, lod_params  # noqa: E402

LIMIT = 485139  # the largest fixture committed before this one (raht_golden.npz)


class RangeCheck:
    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="lift_range_")
        self.exe = lec.build_range_check(self.dir)

    def __call__(self, name, lf, lod, attrs, qp_off, ref_out):
        """exit 0 under the sanitizer and the oracle's output == the reference's"""
        case, out = os.path.join(self.dir, "case.bin"), os.path.join(self.dir, "out.bin")
        lec.write_case_file(case, lf, lod, attrs, qp_off)
        p = subprocess.run([self.exe, case, out], capture_output=True, text=True)
        assert p.returncode == 0, f"{name}: outside the exact range\n{p.stderr[:400]}"
        n, c = attrs.shape
        co, rec, lcp = lec.read_range_output(out, n, c)
        assert np.array_equal(co, ref_out[0]) and np.array_equal(rec, ref_out[1]), f"{name}: oracle != reference"
        if c == 3:
            nl = lf.num_lods
            assert np.array_equal(lcp[:nl], ref_out[2][:nl]), f"{name}: oracle lcp != reference"


def store_case(out, name, field, pk, co, rec, lcp):
    out.params[f"case/{name}"] = repr(pk)
    out.add(f"case/{name}/coeffs", co)
    out.add(f"case/{name}/rec", rec, base=field)
    out.add(f"case/{name}/lcp", lcp)


def geometry(out, r, o, check):
    lods = {}
    for geom in lec.GEOM:
        lod = lh.ref_lod_generate(lec.cloud(geom)[0], lod_params())
        lod["w"] = lod["w"].astype(np.int32)
        lods[geom] = lod
        for k in ("nc", "ni", "w", "indexes", "npl"):
            out.add(f"geom/{geom}/{k}", lod[k])
        out.add(f"geom/{geom}/qp_off", lec.qp_off(len(lod["nc"])))
        print(geom, "npl", list(lod["npl"]))
    assert len(lods["r1500"]["npl"]) == 6 and len(lods["r300"]["npl"]) == 10
    assert len(set(lods["r300"]["npl"])) < 10   # repeated sizes: empty levels from the reference itself
    lcp_seen = {"lcp_pos": set(), "lcp_neg": set()}
    both_clips = 0
    for name, geom, field, c, bd, qp, chroma, qp_off in lec.geometry_cases():
        lod = lods[geom]
        attrs = lec.field_attrs(geom, field)
        if f"field/{geom}/{field}/0" not in out.index:
            out.add(f"field/{geom}/{field}", attrs)
        pk = dict(qp=qp, chroma_offset=chroma, bitdepth=bd, lcp=(c == 3))
        lf = lift_params(lod["npl"], **pk)
        ref_out = lh.lift(r, True, lf, lod, attrs, qp_off=qp_off)
        check(name, lf, lod, attrs, qp_off, ref_out)
        co, rec, lcp = ref_out
        inv = lh.lift(o, False, lf, lod, attrs, coeffs=co, lcp=lcp, qp_off=qp_off)[1]
        assert np.array_equal(inv, rec), name
        # the edge the case is there for
        raw0, qp0, raw1, qp1 = lec.effective_qps(lf, lod["indexes"], qp_off)
        sname = name.rsplit("/", 1)[1]
        if sname in ("qpm10", "qpmax20"):
            assert (raw0 != qp0).any(), name
        if sname in ("chroma_lo", "chroma_hi") and c >= 2:
            assert (raw0 == qp0).all() and (raw1 != qp1).any(), name
        if sname == "qpoff":
            # (at 16 bits max_qp is 99: 30 + 60 stays below it, the second component still passes it)
            assert (raw0 < 4).any() and ((raw0 > lf.max_qp).any() or qp + 60 <= lf.max_qp), name
            assert (raw1 < 4).any() and (raw1 > lf.max_qp).any(), name
        if field.startswith("bin") and sname in ("qpmax", "qpmax20", "chroma_hi"):
            assert (rec == 0).any() and (rec == (1 << bd) - 1).any(), f"{name}: a write-back clip is not reached"
            both_clips += 1
        if field in lcp_seen:
            lcp_seen[field] |= set(int(v) for v in lcp[:len(lod["npl"])])
        if qp_off is not None:
            assert np.array_equal(qp_off, lec.qp_off(len(lod["nc"])))
            pk["qp_off"] = True
        store_case(out, name, f"field/{geom}/{field}", pk, co, rec, lcp)
    assert both_clips > 0
    assert 8 in lcp_seen["lcp_pos"], lcp_seen
    assert -8 in lcp_seen["lcp_neg"], lcp_seen
    print("lcp tables reach", {k: sorted(v) for k, v in lcp_seen.items()})


def synthetic(out, r, o, check):
    structs = {}
    for table, npl in lec.TABLES.items():
        s = structs[table] = lec.synth_structure(npl, lambda nc, d: lh.compute_weights(r, nc, d))
        s_o = lec.synth_structure(npl, lambda nc, d: lh.compute_weights(o, nc, d))
        for k in ("nc", "ni", "w", "indexes", "npl"):
            assert np.array_equal(s[k], s_o[k]), (table, k)
            out.add(f"synth/{table}/{k}", s[k])
        # every neighbour in a coarser level (the reference's assert, PCCTMC3Common.h:805)
        start = np.zeros(npl[-1], np.int64)
        for l in range(1, len(npl)):
            start[npl[l - 1]:npl[l]] = npl[l - 1]
        for j in range(3):
            used = s["nc"] > j
            assert (s["ni"][used, j] < start[used]).all(), table
    for name, table, c, lname, layers in lec.synthetic_cases():
        s = structs[table]
        n = int(s["npl"][-1])
        bits = lec.SYNTH_BD
        attrs = lec.synth_attrs(n, c, bits)
        if f"field/synth/{table}/c{c}/0" not in out.index:
            out.add(f"field/synth/{table}/c{c}", attrs)
        pk = dict(bitdepth=lec.SYNTH_BD, lcp=(c == 3), layers=layers)
        lf = lift_params(s["npl"], **pk)
        ref_out = lh.lift(r, True, lf, s, attrs)
        check(name, lf, s, attrs, None, ref_out)
        co, rec, lcp = ref_out
        inv = lh.lift(o, False, lf, s, attrs, coeffs=co, lcp=lcp)[1]
        assert np.array_equal(inv, rec), name
        store_case(out, "synth/" + name, f"field/synth/{table}/c{c}", pk, co, rec, lcp)


def weights(out, r, o):
    nc, d = lec.weight_rows()
    assert len(nc) == 1864
    nr, wr = lh.compute_weights(r, nc, d)
    no, wo = lh.compute_weights(o, nc, d)
    # reference and oracle agree on EVERY entry, those beyond the kept count included: the tests compare all
    assert np.array_equal(nr, no) and np.array_equal(wr, wo)
    for i in range(len(nc)):
        if nr[i] >= 1:
            assert int(wr[i, :nr[i]].astype(np.int64).sum()) == 256, i
    out.extra["weights/nc_in"] = nc
    out.extra["weights/dist2"] = d
    out.extra["weights/nc"] = nr
    out.extra["weights/w"] = wr


def main():
    r, o = ol.ref(), ol.oracle()
    check = RangeCheck()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lift_edges_golden.npz")
    out = lec.FixtureWriter()
    geometry(out, r, o, check)
    synthetic(out, r, o, check)
    weights(out, r, o)
    out.save(path)
    size = os.path.getsize(path)
    print("wrote", path, "cases", len(out.params), "bytes", size)
    # (over the limit: the 12-bit fields go first, then the 300-point cloud for one component)
    assert size <= LIMIT, f"{size} bytes: over the limit of {LIMIT}"


if __name__ == "__main__":
    main()
