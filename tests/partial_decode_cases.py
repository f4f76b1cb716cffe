"""The committed fixture of the partial (spatially scalable) decode, tests/golden/partial_decode_golden.npz
(TEST INFRASTRUCTURE; written by tests/golden/make_partial_decode_golden.py from the compiled reference).

As in lod_golden.npz the inputs are regenerated from seeds (mpeg_pcc_tmc13_amd.synth) and the reference's large
outputs are stored as SHA-256 digests: per case the cloud's recipe, m, N, the LoD sizes, the coefficients the
decoder consumes, the digest of the reference's LoD structure and of its decoded attributes.  The small cases
(FULL) carry the structure and the attributes in full as well."""
import ast
import functools
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partial_decode_golden.npz")

# name, cloud (kind, points, seed, bits), m, max_neigh_range, lifting parameters, centred
CASES = [
    ("dense_m0", ("dense", 20000, 41, 8), 0, 5, dict(qp=34, chroma_offset=-1), False),
    ("dense_m1", ("dense", 40000, 42, 8), 1, 5, dict(qp=34, chroma_offset=-1), False),
    ("dense_m2", ("dense", 60000, 43, 9), 2, 5, dict(qp=28, chroma_offset=0), False),
    ("dense_m3_nolcp", ("dense", 60000, 44, 9), 3, 2, dict(qp=34, chroma_offset=-1, lcp=False), False),
    ("dense_m2_centred", ("dense", 50000, 45, 8), 2, 5, dict(qp=34, chroma_offset=-1), True),
    ("dense_m2_small", ("dense", 20000, 49, 8), 2, 5, dict(qp=31, chroma_offset=1), False),
    ("dense_m1_layers", ("dense", 30000, 46, 8), 1, 2, dict(layers=[(30, -1), (36, 1), (26, 0)]), False),
    ("lidar_m1", ("lidar", 20000, 47, 0), 1, 5, dict(qp=28, chroma_offset=0), False),
    ("lidar_m3", ("lidar", 40000, 48, 0), 3, 2, dict(qp=34, chroma_offset=0), False),
    ("tiny_m2", ("dense", 4000, 50, 6), 2, 5, dict(qp=30, chroma_offset=-1), False),
    ("tiny_m1_lidar", ("lidar", 3000, 51, 0), 1, 5, dict(qp=28, chroma_offset=0), False),
]
NAMES = [c[0] for c in CASES]
# stored with the reference's structure and attributes in full
FULL = ["tiny_m2", "tiny_m1_lidar"]
# same first level, same LoD parameters, same component count: one ragged device batch
BATCH = ["dense_m2", "dense_m2_centred", "dense_m2_small"]
LOD_KEYS = ("npl", "indexes", "nc", "ni", "w")


def make_cloud(spec):
    from mpeg_pcc_tmc13_amd import synth
    kind, n, seed, bits = spec
    if kind == "dense":
        return synth.dense_cloud(n, seed=seed, bits=bits)
    return synth.lidar_cloud(n, seed=seed)


def partial_cloud(xyz, m, centred=False):
    """the positions decodeGeometryOctreeScalable leaves: nodes of size 2^m in decoded (Morton) order,
    one point each; `centred`: the first eighth as direct-coded points would come out (masked only),
    the octree's nodes behind them, moved to the node centre"""
    from mpeg_pcc_tmc13_amd import synth
    if m == 0:
        return np.ascontiguousarray(xyz, dtype=np.int32).copy()
    order = np.argsort(synth.morton_codes(xyz), kind="stable")
    q = (xyz[order] >> m) << m
    _, first = np.unique(q, axis=0, return_index=True)
    q = q[np.sort(first)]
    if centred:
        k = len(q) // 8
        q[k:] += 1 << (m - 1)
    return np.ascontiguousarray(q, dtype=np.int32)


def live_weights(lod):
    """the weights with the slots beyond the neighbour count as 0 (the reference leaves the raw squared distance
    of a pruned neighbour there, nobody reads it)"""
    live = np.arange(3)[None, :] < np.asarray(lod["nc"])[:, None]
    return np.where(live, np.asarray(lod["w"]).astype(np.uint64), 0).astype(np.int64)


def lod_digest(lod):
    h = hashlib.sha256()
    for k in ("npl", "indexes", "nc", "ni"):
        h.update(np.ascontiguousarray(np.asarray(lod[k]).astype(np.int64)).tobytes())
    h.update(np.ascontiguousarray(live_weights(lod)).tobytes())
    return h.hexdigest()


def attrs_digest(attrs):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(attrs).astype(np.int64)).tobytes()).hexdigest()


_g = None


def golden():
    global _g
    if _g is None:
        _g = np.load(GOLDEN)
    return _g


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(xyz [P,3] (regenerated), N, m, npl, lod_sha, attrs_sha, coeffs [P,c] int32, lcp int8[32],
    lift (keyword arguments of lift_params), max_neigh_range; lod / attrs: the reference's structure and decoded
    attributes in full for the FULL cases, else None)"""
    g = golden()
    _, spec, m, rng, _, centred = CASES[NAMES.index(name)]
    assert ast.literal_eval(str(g[name + "/cloud"])) == (spec, m, centred), "fixture made from another recipe"
    full_xyz = make_cloud(spec)[0]
    xyz = partial_cloud(full_xyz, m, centred)
    assert len(full_xyz) == int(g[name + "/N"]) and len(xyz) == int(g[name + "/P"]), "synth drifted from the fixture"
    full = name + "/ni" in g.files
    return dict(xyz=xyz, N=len(full_xyz), m=m, npl=g[name + "/npl"], lod_sha=str(g[name + "/lod_sha"]),
                attrs_sha=str(g[name + "/attrs_sha"]), coeffs=g[name + "/coeffs"].astype(np.int32), lcp=g[name + "/lcp"],
                lift=ast.literal_eval(str(g[name + "/lift"])), max_neigh_range=rng,
                lod={k: g[f"{name}/{k}"] for k in LOD_KEYS} if full else None,
                attrs=g[name + "/attrs"].astype(np.int32) if full else None)


def assert_lod(got, c, msg=""):
    """`got` is the reference's structure of case `c` (weights compared for the neighbours that exist)"""
    if c["lod"] is not None:
        import emu_lod_loader
        emu_lod_loader.assert_same_lod(got, c["lod"], msg)
    np.testing.assert_array_equal(got["npl"], c["npl"], err_msg=f"{msg} npl")
    assert lod_digest(got) == c["lod_sha"], f"{msg}: LoD structure differs from the reference's"


def assert_attrs(got, c, msg=""):
    if c["attrs"] is not None:
        np.testing.assert_array_equal(got, c["attrs"], err_msg=msg)
    assert attrs_digest(got) == c["attrs_sha"], f"{msg}: decoded attributes differ from the reference's"


def lod_params_of(c):
    from mpeg_pcc_tmc13_amd import lod_params
    lp = lod_params()
    lp.scalable_lifting_enabled_flag = 1
    lp.max_neigh_range_minus1 = c["max_neigh_range"] - 1
    return lp


def lift_params_of(c, npl=None):
    from mpeg_pcc_tmc13_amd import lift_params
    return lift_params(c["npl"] if npl is None else npl, scalable=True, **c["lift"])


def quant_weights_numpy(npl, N, m):
    """computeQuantizationWeightsScalable restated: the weight of every predictor (8 fractional bits)"""
    npl = np.asarray(npl, dtype=np.int64)
    level = np.searchsorted(npl, np.arange(npl[-1]), side="right")
    qw = (N // npl[level]) << 8
    if m == 0:
        qw[level == len(npl) - 1] = 256
    return qw.astype(np.uint64)
