#!/usr/bin/env python3
"""Generate tests/golden/slice_rdo_golden.npz from the COMPILED REFERENCE: the slice-level inter /
intra decision of reflectance slices coded with attribute inter prediction (encoder option
attrInterIntraSliceRDO, AttributeEncoder.cpp:501-585).

Per case (tests/slice_rdo_cases.py holds the recipes; clouds and frames are regenerated from seeds) the
reference's AttributeEncoder::encode codes the slice twice:
  * option OFF: the inter candidate alone.  Its figures -- distortion = sum |reconstruction - source|,
    byte count = payload minus brick header -- are the inter candidate's of the decision;
  * option ON: the decision.  Stored: abh.enableAttrInterPred after the call (the decision), SHA-256 of
    payload and reconstruction, and the intra candidate's figures, which the call leaves in
    AttributeInterPredParams::distEstimate / rateEstimate.
The generator checks that the stored figures reproduce the decision (the reference's own cost
expression, in Python floats), that the winning candidate's bytes are the payload's, and every candidate's
figures against this repository's CPU oracle + the reference's arithmetic coder
(oracle/_ref/libtmc3_entropy.so), which is the arithmetic the GPU tier repeats on the device.

The harness next to this file (slice_rdo_harness.cpp) is compiled into a temporary directory against the
reference's headers and linked with oracle/_ref/libtmc3_ref.so; it runs only where the reference tree
exists."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
import conftest  # noqa: E402,F401
import lod_helpers as lh  # noqa: E402
import oracle_loader as ol  # noqa: E402
import slice_rdo_cases as sc  # noqa: E402

REF = os.environ.get("GPCC_REFERENCE", "/root/reference")


def build_harness(tmp):
    so = os.path.join(tmp, "libslice_rdo_harness.so")
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-O2", "-DNDEBUG", "-std=c++11", "-fPIC", "-shared", "-DTMC3_h", "-w",
           "-I" + REF, "-I" + os.path.join(REF, "tmc3"), "-I" + os.path.join(REF, "dependencies", "nanoflann"),
           "-I" + os.path.join(REF, "dependencies", "schroedinger"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(HERE, "slice_rdo_harness.cpp"), "-o", so,
           "-L" + ref_dir, "-ltmc3_ref", "-Wl,-rpath," + ref_dir]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(so)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
    lib.slice_rdo_case.restype = C.c_int
    lib.slice_rdo_case.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, i32p, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, i32p, i32p, C.c_int32, i32p, i32p, C.c_int32, C.c_int32, C.c_int32, i32p,
                                   u8p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int32)]
    return lib


def run_case(lib, inp, rdo):
    """-> dict(recon [n], payload bytes, inter_after, abh_size, dist_after, rate_after)"""
    n = len(inp["xyz"])
    layers = np.array(inp["layers"], np.int32)
    recon = np.zeros(n, np.int32)
    pay = np.zeros(n * 8 + 4096, np.uint8)
    inter_after, abh_size, rate = C.c_int32(), C.c_int32(), C.c_int32()
    dist = C.c_double()
    ln = lib.slice_rdo_case(C.addressof(inp["lod_inter"]), C.addressof(inp["lod_intra"]), int(inp["seed_cache"]), int(rdo),
                            layers, len(layers), sc.BITDEPTH, inp["direct"], sc.THRESHOLD, inp["xyz"].reshape(-1),
                            inp["attrs"].reshape(-1), n, inp["xyz_ref"].reshape(-1), inp["attrs_ref"].reshape(-1),
                            len(inp["xyz_ref"]), inp["search_range"], inp["frame_distance"], recon, pay, pay.size,
                            C.byref(inter_after), C.byref(abh_size), C.byref(dist), C.byref(rate))
    assert 0 < ln <= pay.size, ln
    return dict(recon=recon, payload=pay[:ln].tobytes(), inter_after=inter_after.value, abh_size=abh_size.value,
                dist_after=dist.value, rate_after=rate.value)


def oracle_candidate(inp, inter):
    """one candidate through this repository's CPU checkers -> (values [n,1], recon [n,1], dist, bytes)"""
    r = ol.oracle()
    xyz, attrs = inp["xyz"], inp["attrs"]
    if inter:
        lod = lh.oracle_lod_generate_inter(xyz, inp["xyz_ref"], inp["lod_inter"], inp["search_range"],
                                           inp["frame_distance"])
    else:
        lod = lh.oracle_lod_generate(xyz, inp["lod_intra"])
    p = sc.transform_params(inp, lod["npl"])
    if inp["transform"] == 2:
        if inter:
            v, rec = lh.lift_inter(r, True, p, lod, attrs, inp["attrs_ref"])
        else:
            v, rec, _ = lh.lift(r, True, p, lod, attrs)
    else:
        if inter:
            v, rec, _ = lh.pred_inter(True, p, lod, inp["attrs_ref"], attrs=attrs)
        else:
            v, rec, _, _ = lh.oracle_pred(True, p, lod, attrs=attrs)
    n = len(xyz)
    runs, vals, trailing = lh.oracle_zero_run_pack(v, n, 1, 0)
    bins = lh.oracle_binarise_symbols(runs, vals, trailing, 1)
    coded = lh.ref_entropy_encode_bins(bins, n)
    return v, rec, int(np.abs(rec.astype(np.int64) - attrs).sum()), len(coded)


def python_choice(dist, nbytes, init_qp_minus4):
    """AttributeInterPredParams::setLambda / getCost in Python floats (IEEE doubles, the same operations)"""
    q = int(init_qp_minus4 / 3)  # C++ integer division truncates towards zero
    lam = (0.85 * 2.0 ** q) ** 0.5
    cost = [float(dist[0]) + lam * int(nbytes[0]), float(dist[1]) + lam * int(nbytes[1])]
    return cost[0] > cost[1], cost


def main():
    assert os.path.isdir(os.path.join(REF, "tmc3")), "the reference tree is needed to regenerate this fixture"
    out = {"names": np.array(sc.NAMES)}
    check_oracle = "--no-oracle" not in sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_harness(tmp)
        for name in sc.NAMES:
            inp = sc.inputs(name)
            n = len(inp["xyz"])
            off = run_case(lib, inp, rdo=False)
            on = run_case(lib, inp, rdo=True)
            assert off["inter_after"] == 1
            dist = np.array([np.abs(off["recon"].astype(np.int64) - inp["attrs"][:, 0]).sum(), int(on["dist_after"])], np.int64)
            assert float(dist[1]) == on["dist_after"]
            nbytes = np.array([len(off["payload"]) - off["abh_size"], on["rate_after"]], np.int64)
            intra_wins = on["inter_after"] == 0
            win, cost = python_choice(dist, nbytes, inp["init_qp_minus4"])
            assert win == intra_wins, (name, cost, intra_wins)
            assert len(on["payload"]) - on["abh_size"] == nbytes[int(intra_wins)], name
            if not intra_wins:
                assert on["payload"] == off["payload"] and np.array_equal(on["recon"], off["recon"]), name
            if check_oracle:
                for k in (0, 1):
                    v, rec, d, b = oracle_candidate(inp, inter=k == 0)
                    assert (d, b) == (int(dist[k]), int(nbytes[k])), (name, k, d, b, dist, nbytes)
                    if k == int(intra_wins):
                        assert np.array_equal(rec[:, 0], on["recon"]), (name, "winner's reconstruction")
            out[name + "/n"] = np.int64(n)
            out[name + "/n_ref"] = np.int64(len(inp["xyz_ref"]))
            out[name + "/init_qp_minus4"] = np.int64(inp["init_qp_minus4"])
            out[name + "/intra_wins"] = np.bool_(intra_wins)
            out[name + "/dist"] = dist
            out[name + "/bytes"] = nbytes
            out[name + "/cost"] = np.array(cost, np.float64)
            out[name + "/payload_sha"] = np.array(sc.digest(np.frombuffer(on["payload"], np.uint8), np.uint8))
            out[name + "/recon_sha"] = np.array(sc.digest(on["recon"]))
            if name in sc.FULL:
                out[name + "/payload"] = np.frombuffer(on["payload"], np.uint8)
                out[name + "/recon"] = on["recon"].astype(np.uint8)
            print(name, "n", n, "intra wins" if intra_wins else "inter wins", "dist", dist.tolist(), "bytes",
                  nbytes.tolist(), "cost %.3f %.3f" % tuple(cost))
    path = os.path.join(HERE, "slice_rdo_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
