"""The cases of tests/golden/ref_crop_golden.npz (TEST INFRASTRUCTURE): the previous frame cropped to the bounding
box of the current slice, as the reference does in front of its lifting and predicting coders when attribute inter
prediction is on (encoder.cpp:1215-1236, decoder.cpp:926-947: computeBoundingBox, Box3::contains, an ordered
copy of positions and attributes).  Clouds are regenerated from seeds / built by hand here; the fixture holds per
case the slices' boxes, the offsets of the cropped frames, SHA-256 digests of the kept positions and attributes --
and the arrays in full for the cases of at most FULL_MAX frame points.  The one case whose input cannot be rebuilt
from numpy alone (two synthetic lidar frames moved into the spherical domain by the reference) has its input in
the fixture as well.

Every coordinate lies in [0, 2^21), the entries' domain; attributes fit the reference's 16-bit attribute type."""
import hashlib
import os

import numpy as np

import conftest  # noqa: F401  (makes the package importable)
from mpeg_pcc_tmc13_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_crop_golden.npz")
FULL_MAX = 4096
TILE = 1024  # kRefCropTile

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 3 * 1024 + 1)
PATTERNS = ("all", "none", "alternating", "first", "last")
LO, HI = 100, 200  # the box of the hand-built cases: [LO, HI]^3

LIDAR_POINTS, LIDAR_SLICES, LIDAR_SEEDS = 3000, 8, (1, 2)


def _box_slice(rng, extra=6):
    """a current slice whose bounding box is exactly [LO, HI]^3: the two corners first and last, anything between"""
    mid = rng.integers(LO, HI + 1, (extra, 3))
    return np.concatenate([[[LO, HI, LO]], mid, [[HI, LO, HI]]]).astype(np.int32)


def _pattern_frame(n, pattern, c, seed):
    """n frame points; which of them lie inside [LO, HI]^3 is the pattern.  A point outside differs from the box in
    ONE component only, by any amount, below or above"""
    rng = np.random.default_rng(seed)
    xyz = rng.integers(LO, HI + 1, (n, 3))
    idx = np.arange(n)
    inside = {"all": idx >= 0, "none": idx < 0, "alternating": idx % 2 == 0, "first": idx == 0,
              "last": idx == n - 1}[pattern]
    out = np.flatnonzero(~inside)
    comp = rng.integers(0, 3, len(out))
    below = rng.integers(0, 2, len(out)) == 0
    xyz[out, comp] = np.where(below, rng.integers(0, LO, len(out)), rng.integers(HI + 1, 2 * HI, len(out)))
    attrs = rng.integers(0, 1 << 16, (n, c))
    return xyz.astype(np.int32), attrs.astype(np.int32), _box_slice(rng)


def _faces_frame(c):
    """a point on each of the six faces, on edges and corners (kept), one step outside each face (dropped)"""
    m = (LO + HI) // 2
    pts = []
    for k in range(3):
        for v, keep_step in ((LO, -1), (HI, +1)):
            p = [m, m + 1, m + 2]
            p[k] = v
            pts.append(list(p))          # on the face
            p[k] = v + keep_step
            pts.append(list(p))          # one step outside
    pts += [[LO, LO, LO], [HI, HI, HI], [LO, HI, m], [LO - 1, LO, LO], [HI, HI, HI + 1], [HI + 1, HI + 1, HI + 1]]
    xyz = np.array(pts, np.int32)
    attrs = (np.arange(len(xyz) * c).reshape(-1, c) * 37 + 5).astype(np.int32)
    return xyz, attrs, _box_slice(np.random.default_rng(9))


def _one_point(c):
    """a current slice of ONE point: the box is that point; the frame holds it twice among its 26 neighbours"""
    p = np.array([150, 151, 152], np.int32)
    d = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([p + d, [p]]).astype(np.int32)
    attrs = (np.arange(len(xyz) * c).reshape(-1, c) + 1000).astype(np.int32)
    return xyz, attrs, p.reshape(1, 3)


RAGGED_SLICES, RAGGED_FRAME = 300, 5000


def _ragged():
    """300 current slices of 1..60 points against one frame of 5 000 points in a 64^3 cube: every 20th slice lies
    outside the cube (keeps nothing), the others are boxes of every size inside it"""
    fx, fa = synth.random_cloud(RAGGED_FRAME, seed=500, bits=6, c=1, bitdepth=16)
    rng = np.random.default_rng(501)
    sizes = rng.integers(1, 61, RAGGED_SLICES)
    parts = []
    for s, n in enumerate(sizes):
        if s % 20 == 0:
            parts.append(rng.integers(1000 + 10 * s, 1000 + 10 * s + 9, (n, 3)))
        else:
            ext = int(rng.integers(1, 40))
            org = rng.integers(0, 64 - ext, 3)
            parts.append(org + rng.integers(0, ext + 1, (n, 3)))
    cur = np.concatenate(parts).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return fx, fa, cur, off


# name -> recipe
CASES = {}
for _n in SIZES:
    for _p in PATTERNS:
        CASES[f"{_p}_{_n}_c1"] = ("pattern", _n, _p, 1)
    CASES[f"alternating_{_n}_c3"] = ("pattern", _n, "alternating", 3)
for _c in (1, 3):
    CASES[f"faces_c{_c}"] = ("faces", _c)
    CASES[f"one_point_c{_c}"] = ("one_point", _c)
CASES["unaligned_1025_c1"] = ("pattern", 1025, "alternating", 1, "unaligned")
CASES["unaligned_3073_c3"] = ("pattern", 3073, "alternating", 3, "unaligned")
CASES["ragged300"] = ("ragged",)
CASES["lidar8"] = ("lidar",)
NAMES = list(CASES)

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = np.load(GOLDEN)
    return _golden


def inputs(name, stored=None):
    """-> dict(frame_xyz [nf, 3], frame_attrs [nf, c], xyz [n, 3] the current slices, offsets int64 [slices + 1],
    unaligned: the frame's arrays are to start one point behind a 16-byte boundary).  stored: where the lidar case's
    input comes from (default: the fixture)"""
    rec = CASES[name]
    unaligned = rec[-1] == "unaligned"
    if rec[0] == "pattern":
        fx, fa, cur = _pattern_frame(rec[1], rec[2], rec[3], 7000 + 13 * rec[1] + PATTERNS.index(rec[2]))
    elif rec[0] == "faces":
        fx, fa, cur = _faces_frame(rec[1])
    elif rec[0] == "one_point":
        fx, fa, cur = _one_point(rec[1])
    elif rec[0] == "ragged":
        fx, fa, cur, off = _ragged()
        return dict(name=name, frame_xyz=fx, frame_attrs=fa, xyz=cur, offsets=off, unaligned=False)
    else:
        g = golden() if stored is None else stored
        fx, fa, cur = g["lidar8/in_frame_xyz"], g["lidar8/in_frame_attrs"], g["lidar8/in_xyz"]
        off = np.linspace(0, len(cur), LIDAR_SLICES + 1).astype(np.int64)
        return dict(name=name, frame_xyz=fx, frame_attrs=fa, xyz=cur, offsets=off, unaligned=False)
    return dict(name=name, frame_xyz=fx, frame_attrs=fa, xyz=cur, offsets=np.array([0, len(cur)], np.int64),
                unaligned=unaligned)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def crop_numpy(xyz, offsets, frame_xyz, frame_attrs):
    """the numpy restatement -> (bbox [slices, 6], ref_offsets int64 [slices + 1], positions, attributes)"""
    boxes, ox, oa, ro = [], [], [], [0]
    for s in range(len(offsets) - 1):
        p = xyz[offsets[s]:offsets[s + 1]]
        mn, mx = p.min(0), p.max(0)
        keep = ((frame_xyz >= mn) & (frame_xyz <= mx)).all(1)
        boxes.append(np.concatenate([mn, mx]))
        ox.append(frame_xyz[keep])
        oa.append(frame_attrs[keep])
        ro.append(ro[-1] + int(keep.sum()))
    return (np.stack(boxes).astype(np.int32), np.array(ro, np.int64), np.concatenate(ox).astype(np.int32),
            np.concatenate(oa).astype(np.int32))


def case(name):
    """inputs(name) plus the reference's results: bbox [slices, 6], ref_offsets [slices + 1], xyz_sha, attrs_sha,
    and ref_xyz / ref_attrs in full where the fixture has them"""
    g = golden()
    c = inputs(name)
    c.update(bbox=g[name + "/bbox"], ref_offsets=g[name + "/ref_offsets"], xyz_sha=str(g[name + "/xyz_sha"]),
             attrs_sha=str(g[name + "/attrs_sha"]))
    for k in ("ref_xyz", "ref_attrs"):
        if f"{name}/{k}" in g.files:
            c[k] = g[f"{name}/{k}"]
    return c


def check(c, bbox, ref_offsets, ref_xyz, ref_attrs):
    """a result against the fixture"""
    np.testing.assert_array_equal(ref_offsets, c["ref_offsets"])
    if bbox is not None:
        np.testing.assert_array_equal(np.asarray(bbox).reshape(-1, 6), c["bbox"])
    k = int(c["ref_offsets"][-1])
    assert len(ref_xyz) == k and len(ref_attrs) == k
    if "ref_xyz" in c:
        np.testing.assert_array_equal(ref_xyz, c["ref_xyz"])
        np.testing.assert_array_equal(ref_attrs, c["ref_attrs"])
    assert digest(ref_xyz) == c["xyz_sha"]
    assert digest(ref_attrs) == c["attrs_sha"]
