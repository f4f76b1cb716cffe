#!/usr/bin/env python3
"""Generate tests/golden/partial_decode_golden.npz from the COMPILED REFERENCE: the spatially
scalable ("partial") decode of scalable-lifting slices, minGeomNodeSizeLog2 = m > 0.

Per case: a synthetic cloud of N points is encoded by the reference's lifting encoder
(makeAttributeEncoder, scalable lifting); the cloud a geometry decoder leaves when it stops m
octree levels early (positions masked to multiples of 2^m, duplicates removed in decoded order, for
one case partly centred by 2^(m-1)) goes through the reference's AttributeLods::generate(aps, abh,
N - 1, m, ...) and AttributeDecoder::decode(..., N - 1, m, ...).  The clouds are regenerated from seeds
(tests/partial_decode_cases.py holds the recipes).  Stored per case: the recipe, N, P, the parameters, the
LoD sizes, the first P rows of the coefficient sequence of the full encode (what the decoder consumes; from
the reference's own lifting templates over the reference's full structure, ref_lift_forward), the
last-component-prediction coefficients of the brick header, and SHA-256 digests of the reference's partial
LoD structure (npl, indexes, neighbour counts / indices, weights of the neighbours that exist) and of its
decoded attributes -- for the small cases the structure and the attributes in full as well.

The harness next to this file (partial_decode_harness.cpp) is compiled into a temporary directory
against the reference's headers and linked with oracle/_ref/libtmc3_ref.so; it runs only where the
reference tree exists.  One m = 0 case cross-checks the generator against the pinned whole-slice
path."""
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
import partial_decode_cases as pc  # noqa: E402  (the cases, the clouds' recipes, the digests)
from mpeg_pcc_tmc13_amd import lift_params, lod_params  # noqa: E402

REF = os.environ.get("GPCC_REFERENCE", "/root/reference")

def make_lod_params(max_neigh_range):
    lp = lod_params()
    lp.scalable_lifting_enabled_flag = 1
    lp.max_neigh_range_minus1 = max_neigh_range - 1
    return lp


def build_harness(tmp):
    so = os.path.join(tmp, "libpartial_decode_harness.so")
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    cmd = ["g++", "-O2", "-DNDEBUG", "-std=c++11", "-fPIC", "-shared", "-DTMC3_h", "-w",
           "-I" + REF, "-I" + os.path.join(REF, "tmc3"), "-I" + os.path.join(REF, "dependencies", "nanoflann"),
           "-I" + os.path.join(REF, "dependencies", "schroedinger"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(HERE, "partial_decode_harness.cpp"), "-o", so,
           "-L" + ref_dir, "-ltmc3_ref", "-Wl,-rpath," + ref_dir]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(so)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
    i8p = np.ctypeslib.ndpointer(np.int8, flags="C_CONTIGUOUS")
    lib.partial_decode_case.restype = C.c_int
    lib.partial_decode_case.argtypes = [C.c_void_p, i32p, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, C.c_int32,
                                        C.c_int32, i32p, C.c_int32, C.c_int32, i32p, i32p, u64p, i32p, i32p,
                                        C.POINTER(C.c_int32), i32p, i8p]
    return lib


def run_case(lib, lp, lf, xyz, attrs, part, m):
    N, c = attrs.shape
    P = len(part)
    layers = np.array([[lf.layer_qp[i][0], lf.layer_qp[i][1]] for i in range(lf.num_qp_layers)], np.int32)
    nc = np.zeros(P, np.int32)
    ni = np.zeros((P, 3), np.int32)
    w = np.zeros((P, 3), np.uint64)
    idx = np.zeros(P, np.int32)
    npl = np.zeros(32, np.int32)
    nl = C.c_int32()
    dec = np.zeros((P, c), np.int32)
    lcp = np.zeros(32, np.int8)
    ln = lib.partial_decode_case(C.addressof(lp), layers.reshape(-1), len(layers), lf.bitdepth,
                                 lf.last_component_prediction_enabled_flag,
                                 np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1),
                                 np.ascontiguousarray(attrs, dtype=np.int32).reshape(-1), N, c, part.reshape(-1), P, m,
                                 nc, ni.reshape(-1), w.reshape(-1), idx, npl, C.byref(nl), dec.reshape(-1), lcp)
    assert ln > 0, ln
    return dict(nc=nc, ni=ni, w=w, indexes=idx, npl=npl[:nl.value].copy()), dec, lcp


def main():
    assert os.path.isdir(os.path.join(REF, "tmc3")), "the reference tree is needed to regenerate this fixture"
    r = ol.ref()
    out = {"names": np.array(pc.NAMES)}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_harness(tmp)
        for name, spec, m, rng, pk, centred in pc.CASES:
            xyz, attrs = pc.make_cloud(spec)
            N, c = attrs.shape
            pk = dict(pk)
            lcp_on = pk.pop("lcp", True) and c == 3
            lp = make_lod_params(rng)
            # the coefficient sequence of the full encode, in coding order
            full = lh.ref_lod_generate(xyz, lp)
            lf = lift_params(full["npl"], lcp=lcp_on, scalable=True, **pk)
            co, rec, lcp_enc = lh.lift(r, True, lf, full, attrs)
            part = pc.partial_cloud(xyz, m, centred)
            P = len(part)
            lod, dec, lcp = run_case(lib, lp, lf, xyz, attrs, part, m)
            if lcp_on:
                assert np.array_equal(lcp[:len(full["npl"])], lcp_enc[:len(full["npl"])]), name
            if m == 0:
                # the generator against the pinned whole-slice path
                for k in ("npl", "indexes", "nc", "ni"):
                    assert np.array_equal(lod[k], full[k]), (name, k)
                assert np.array_equal(dec, rec), name
            out[name + "/cloud"] = np.array(repr((spec, m, centred)))
            out[name + "/N"] = np.int64(N)
            out[name + "/P"] = np.int64(P)
            out[name + "/lift"] = np.array(repr(dict(pk, lcp=lcp_on)))
            out[name + "/npl"] = lod["npl"].astype(np.int32)
            out[name + "/lod_sha"] = np.array(pc.lod_digest(lod))
            out[name + "/attrs_sha"] = np.array(pc.attrs_digest(dec))
            out[name + "/coeffs"] = _narrow(co[:P])
            out[name + "/lcp"] = lcp
            if name in pc.FULL:
                for k in ("indexes", "nc", "ni"):
                    out[f"{name}/{k}"] = lod[k].astype(np.int32)
                out[name + "/w"] = pc.live_weights(lod).astype(np.int32)
                out[name + "/attrs"] = dec.astype(np.uint8 if dec.max() < 256 else np.int32)
            print(name, "N", N, "P", P, "m", m, "lods", len(lod["npl"]), "nonzero", np.count_nonzero(co[:P]))
    path = os.path.join(HERE, "partial_decode_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


def _narrow(a):
    return a.astype(np.int16) if np.abs(a).max() < 32768 else a


if __name__ == "__main__":
    main()
