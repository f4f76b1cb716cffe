"""Case table of the lifting transform's edge tests (TEST INFRASTRUCTURE): what
tests/golden/make_lift_edges_golden.py stores in lift_edges_golden.npz and what
tests/test_oracle_lift_edges.py / tests/test_gpu_lift_edges.py walk.

(a) geometry cases: two small clouds whose LoD structure the reference's
    AttributeLods::generate gives (six levels; ten levels with repeated sizes),
    attribute fields at the edges of the value range, and QP parameter sets at
    and beyond every clamp of the quantiser's QP;
(b) synthetic structures: LoD size tables chosen for the wavefront paths of the
    last-component-prediction sums and for the host's replay of the reference's
    running `quantLayer` / `lod` counters (empty levels; more QP layers than
    levels);
(c) a table of squared-distance triples for PCCPredictor::computeWeights.

Every attribute value stays inside the range in which the reference's own
lifting arithmetic is exact ("Lifting transform": `scaled *
iQuantWeight` wraps once a coefficient reaches about 2^15 attribute units); the
generator checks that for every case before it writes the fixture."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lift_edges_golden.npz")

# ---- (a) geometry -----------------------------------------------------------------------------
GEOM = {"r1500": dict(n=1500, seed=5, bits=5),   # six levels
        "r300": dict(n=300, seed=5, bits=9)}     # ten levels, repeated sizes


def max_qp(bd):
    return 51 + 6 * (bd - 8)


def cloud(geom, c=3, bd=8):
    """-> (xyz, full-range random attributes [n, c]); xyz does not depend on c / bd"""
    from mpeg_pcc_tmc13_amd import synth
    return synth.random_cloud(c=c, bitdepth=bd, **GEOM[geom])


def _binary(geom, c, bd):
    n = GEOM[geom]["n"]
    rng = np.random.default_rng(11)
    return np.where(rng.random((n, c)) < 0.5, 0, (1 << bd) - 1).astype(np.int32)


LCP_BD = 8
LCP_A_BITS = 6


def _lcp(geom, sign):
    """second component A, third 2A (last-component coefficient +8) or max - 2A (-8); A is kept
    small so that the int32 products of the coefficient sums do not wrap into noise"""
    n = GEOM[geom]["n"]
    rng = np.random.default_rng(12)
    a = rng.integers(0, 1 << LCP_A_BITS, size=n).astype(np.int32)
    first = rng.integers(0, 1 << LCP_BD, size=n).astype(np.int32)
    third = 2 * a if sign > 0 else ((1 << LCP_BD) - 1) - 2 * a
    return np.stack([first, a, third], axis=1).astype(np.int32)


# The "binary" field (each value 0 or 2^BD - 1: the largest details) at 14 bits stays inside the exact range on
# the 1500-point cloud only: on the sparse 300-point cloud its quantisation weights carry a coefficient past
# it (tests/lift_range_check.c stops at `scaled * iQuantWeight`), so that cloud takes the field at 13 bits.
BINARY_BD = {"r1500": 14, "r300": 13}


def fields(geom):
    """-> [(field name, c, bit depth)]"""
    out = []
    for c in (1, 3):
        for bd in (8, 12, 14):
            out.append((f"rand{bd}_c{c}", c, bd))
        out.append((f"bin{BINARY_BD[geom]}_c{c}", c, BINARY_BD[geom]))
        out.append((f"band16_c{c}", c, 16))
    out.append(("lcp_pos", 3, LCP_BD))
    out.append(("lcp_neg", 3, LCP_BD))
    return out


def field_attrs(geom, field):
    """the attributes of a field on a cloud, int32 [n, c]"""
    name, c, bd = next(f for f in fields(geom) if f[0] == field)
    if name.startswith("rand"):
        return cloud(geom, c, bd)[1]
    if name.startswith("bin"):
        return _binary(geom, c, bd)
    if name.startswith("band"):
        return (cloud(geom, c, 16)[1] >> 2) + 8192
    return _lcp(geom, +1 if name == "lcp_pos" else -1)


def param_sets(bd):
    """-> [(set name, qp, chroma offset, per-point qp_off?)]"""
    mq = max_qp(bd)
    return [("qp4", 4, 0, False),             # lower bound
            ("qpm10", -10, 0, False),         # below the lower clamp
            ("qpmax", mq, 0, False),          # upper bound
            ("qpmax20", mq + 20, 0, False),   # above the upper clamp
            ("chroma_lo", 8, -20, False),     # second component clamped low
            ("chroma_hi", mq - 2, 20, False),  # second component clamped high
            ("qpoff", 30, 0, True)]           # both clamps per point


def qp_off(n):
    return np.random.default_rng(13).integers(-60, 61, size=(n, 2)).astype(np.int32)


def geometry_cases():
    """-> [(case name, geom, field, c, bd, qp, chroma offset, qp_off or None)]"""
    out = []
    for geom in GEOM:
        for field, c, bd in fields(geom):
            for sname, qp, chroma, per_point in param_sets(bd):
                out.append((f"{geom}/{field}/{sname}", geom, field, c, bd, qp, chroma,
                            qp_off(GEOM[geom]["n"]) if per_point else None))
    return out


def effective_qps(lf, indexes, qp_off_, layer=0):
    """(qp of the first, of the second component) per coefficient for one QP layer, before and
    after the clamps -> (raw0, qp0, raw1, qp1)"""
    n = len(indexes)
    o = np.zeros((n, 2), np.int64) if qp_off_ is None else np.asarray(qp_off_, np.int64)[np.asarray(indexes)]
    raw0 = int(lf.layer_qp[layer][0]) + o[:, 0]
    qp0 = np.clip(raw0, 4, lf.max_qp)
    raw1 = int(lf.layer_qp[layer][1]) + o[:, 1] + qp0
    qp1 = np.clip(raw1, 4, lf.max_qp)
    return raw0, qp0, raw1, qp1


# ---- (b) synthetic structures -----------------------------------------------------------------
TABLES = {
    "wave320": [64, 128, 320],                 # every boundary on a wavefront
    "wave300": [64, 128, 300],                 # the same, a partly valid last wavefront
    "straddle": [1, 63, 65, 257, 300],         # wavefronts that straddle levels
    "empty": [1, 1, 1, 1, 2, 5, 5, 70],        # empty levels in front and in the middle
    "one": [7],
    "two": [1, 2],
    "lods27": [1] * 21 + [3, 9, 27, 81, 243, 300],
}
SYNTH_BD = 14


def synth_structure(npl, compute_weights, seed=1):
    """predictors built directly: per point of LoD l >= 1 up to three distinct neighbours below the
    LoD's start, sorted random squared distances below 2^k (k uniform in [1, 30)), weights by
    computeWeights (`compute_weights(nc, dist2) -> (nc, w)`), a random coding order"""
    rng = np.random.default_rng(seed)
    n = npl[-1]
    nc = np.zeros(n, np.int32)
    ni = np.zeros((n, 3), np.int32)
    d = np.zeros((n, 3), np.uint64)
    bounds = [0] + list(npl)
    for l in range(1, len(npl)):
        s, e = bounds[l], bounds[l + 1]
        if s == 0:
            continue
        for i in range(s, e):
            k = min(int(rng.integers(0, 4)), s)
            nc[i] = k
            ni[i, :k] = rng.choice(s, size=k, replace=False)
            d[i, :k] = np.sort(rng.integers(0, 1 << int(rng.integers(1, 30)), size=k).astype(np.uint64))
    nc2, w = compute_weights(nc, d)
    return dict(nc=nc2, ni=ni, w=np.asarray(w).astype(np.int32), indexes=rng.permutation(n).astype(np.int32),
                npl=np.array(npl, np.int32))


def synth_attrs(n, c, bits=SYNTH_BD):
    return np.random.default_rng(2).integers(0, 1 << bits, size=(n, c)).astype(np.int32)


def layer_lists(npl):
    """-> [(name, QP layers)]: one, two, one per LoD, 32 (the most the header allows)"""
    return [("l1", [(4, 0)]),
            ("l2", [(30, -1), (36, 1)]),
            ("lnl", [(20 + i, (i % 3) - 1) for i in range(len(npl))]),
            ("l32", [(10 + 2 * i, 0) for i in range(32)])]


def synthetic_cases():
    """-> [(case name, table, c, layer-list name, layers)]"""
    out = []
    for table, npl in TABLES.items():
        for c in (1, 3):
            for lname, layers in layer_lists(npl):
                out.append((f"{table}/c{c}/{lname}", table, c, lname, layers))
    return out


# ---- (c) computeWeights -----------------------------------------------------------------------
WEIGHT_D0 = (0, 1, 2, 127, 128, 254, 255, 256, 257, 511, 512, 4087, 4088, 4095, 4096, (1 << 20) - 1,
             (1 << 40) + 12345, (1 << 62) - 1, 1 << 62)


def weight_rows():
    """-> (neighbour counts int32 [m], squared distances uint64 [m, 3]): d0 over duplicates (0), the
    rounding that lifts d0 to exactly 256, distances beyond 32 bits; d1 / d2 as sums with {0, 1} or
    multiples {255, 256, 257, 1000} of d0 (the tie d[cnt-1] == d0 << 8 among them); sorted, below
    2^63; every neighbour count"""
    rows = []
    for d0 in WEIGHT_D0:
        for m1 in (0, 1, 255, 256, 257):
            for m2 in (0, 1, 255, 256, 257, 1000):
                d1 = d0 + m1 if m1 < 255 else d0 * m1
                if d1 >= (1 << 63):
                    continue
                d2 = d1 + m2 if m2 < 255 else d0 * m2
                if d2 < d1 or d2 >= (1 << 63):
                    continue
                for nc in (0, 1, 2, 3):
                    rows.append((nc, d0, d1, d2))
    nc = np.array([r[0] for r in rows], np.int32)
    d = np.array([r[1:] for r in rows], np.uint64)
    return nc, d


# ---- the fixture ------------------------------------------------------------------------------
# golden/lift_edges_golden.npz keeps every array by column in the smallest integer type that holds it, all
# columns of one type back to back in one blob, a column that occurs twice once (a QP beyond a clamp gives what
# the bound gives; the chroma-offset sets share the second and third column with them), and a reconstruction
# as its difference to the attribute column where that is shorter.
# Lossless: FixtureWriter.add / Fixture[name] are inverse to each other.
_DTYPES = (np.int8, np.uint16, np.int16, np.int32)


def small(a):
    """-> (code into _DTYPES, `a` in the smallest integer type that holds it)"""
    a = np.asarray(a)
    lo, hi = (int(a.min()), int(a.max())) if a.size else (0, 0)
    if lo >= -128 and hi < 128:
        return 0, a.astype(np.int8)
    if lo >= 0 and hi < (1 << 16):
        return 1, a.astype(np.uint16)
    if lo >= -(1 << 15) and hi < (1 << 15):
        return 2, a.astype(np.int16)
    assert lo >= -(1 << 31) and hi < (1 << 31)
    return 3, a.astype(np.int32)


class FixtureWriter:
    def __init__(self):
        self.blobs = [[] for _ in _DTYPES]
        self.used = [0] * len(_DTYPES)
        self.names, self.rows, self.seen, self.index = [], [], {}, {}
        self.params, self.extra = {}, {}

    def _column(self, name, col, base):
        import zlib
        col = np.asarray(col).astype(np.int64)
        assert name not in self.index, name
        b = -1
        if base is not None:
            delta = col - self.value(base)
            if len(zlib.compress(small(delta)[1].tobytes(), 9)) < len(zlib.compress(small(col)[1].tobytes(), 9)):
                col, b = delta, self.index[base]
        code, data = small(col)
        key = (code, data.tobytes())
        if key not in self.seen:
            self.seen[key] = (self.used[code], len(data))
            self.blobs[code].append(data)
            self.used[code] += len(data)
        off, ln = self.seen[key]
        self.index[name] = len(self.rows)
        self.names.append(name)
        self.rows.append((code, off, ln, b))

    def value(self, name):
        code, off, ln, b = self.rows[self.index[name]]
        v = np.concatenate(self.blobs[code])[off:off + ln].astype(np.int64)
        return v if b < 0 else v + self.value(self.names[b])

    def add(self, name, a, base=None):
        """a [n] or [n, c] (stored as name/0 .. name/c-1); base: the name of an array of the same shape the
        columns may be stored as differences to"""
        a = np.asarray(a)
        if a.ndim == 1:
            self._column(name, a, base)
        else:
            for k in range(a.shape[1]):
                self._column(f"{name}/{k}", a[:, k], None if base is None else f"{base}/{k}")

    def save(self, path, date_time=None):
        """date_time: the time stamp of every member (a zip member carries the time of writing otherwise, and two
        runs differ in those bytes)"""
        out = {f"blob{i}": np.concatenate(b).astype(_DTYPES[i]) if b else np.zeros(0, _DTYPES[i])
               for i, b in enumerate(self.blobs)}
        out["table"] = np.array(self.rows, np.int64).reshape(-1, 4)
        out["names"] = np.array("\n".join(self.names))
        out["params"] = np.array("\n".join(f"{k}\t{v}" for k, v in self.params.items()))
        out.update(self.extra)
        # an .npz as numpy.load reads it, with the zip container's LZMA method (a third smaller than deflate here)
        import io
        import zipfile
        with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
            for k, v in out.items():
                b = io.BytesIO()
                np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
                member = k + ".npy" if date_time is None else zipfile.ZipInfo(k + ".npy", date_time)
                z.writestr(member, b.getvalue(), compress_type=zipfile.ZIP_LZMA)


class Fixture:
    """read access: g[name] -> int32 [n], or [n, c] for an array stored by column; g.params[case key]"""

    def __init__(self, path):
        z = np.load(path)
        self.blobs = [z[f"blob{i}"] for i in range(len(_DTYPES))]
        self.table = z["table"]
        self.names = str(z["names"]).split("\n")
        self.index = {n: i for i, n in enumerate(self.names)}
        self.params = dict(line.split("\t") for line in str(z["params"]).split("\n"))
        self.extra = {k: z[k] for k in z.files if k.startswith("weights/")}
        self.cache = {}

    def __contains__(self, name):
        return name in self.index or name + "/0" in self.index or name in self.extra

    def _column(self, i):
        code, off, ln, b = (int(v) for v in self.table[i])
        v = self.blobs[code][off:off + ln].astype(np.int32)
        return v if b < 0 else v + self._column(b)

    def __getitem__(self, name):
        if name in self.extra:
            return self.extra[name]
        if name not in self.cache:
            if name in self.index:
                v = self._column(self.index[name])
            else:
                cols = []
                while f"{name}/{len(cols)}" in self.index:
                    cols.append(self._column(self.index[f"{name}/{len(cols)}"]))
                if not cols:
                    raise KeyError(name)
                v = np.ascontiguousarray(np.stack(cols, axis=1))
            v.setflags(write=False)
            self.cache[name] = v
        return self.cache[name]

    def cases(self):
        return list(self.params)


def all_cases(g):
    """-> [(case key, lift params, structure, attrs, qp_off or None)] for every case of the table, from the
    fixture `g`"""
    import ast
    from mpeg_pcc_tmc13_amd import lift_params
    out = []
    for name, geom, field, c, bd, qp, chroma, per_point in geometry_cases():
        lod = structure(g, f"geom/{geom}")
        pk = ast.literal_eval(g.params[f"case/{name}"])
        q = g[f"geom/{geom}/qp_off"] if pk.pop("qp_off", False) else None
        assert (q is None) == (per_point is None)
        out.append((f"case/{name}", lift_params(lod["npl"], **pk), lod, g[f"field/{geom}/{field}"], q))
    for name, table, c, lname, layers in synthetic_cases():
        lod = structure(g, f"synth/{table}")
        pk = ast.literal_eval(g.params[f"case/synth/{name}"])
        out.append((f"case/synth/{name}", lift_params(lod["npl"], **pk), lod, g[f"field/synth/{table}/c{c}"], None))
    return out


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def structure(g, prefix):
    """a stored LoD structure as lod_helpers.lift takes it"""
    return dict(nc=i32(g[prefix + "/nc"]), ni=i32(g[prefix + "/ni"]), w=i32(g[prefix + "/w"]),
                indexes=i32(g[prefix + "/indexes"]), npl=i32(g[prefix + "/npl"]))


def write_case_file(path, lf, lod, attrs, qp_off_=None):
    """the raw arrays of one forward lifting case for tests/lift_range_check.c"""
    a = i32(attrs)
    n, c = a.shape
    with open(path, "wb") as f:
        f.write(np.array([n, c, int(qp_off_ is not None)], np.int32).tobytes())
        f.write(bytes(lf))
        for arr in (lod["nc"], lod["ni"], lod["w"], lod["indexes"]):
            f.write(i32(arr).tobytes())
        if qp_off_ is not None:
            f.write(i32(qp_off_).tobytes())
        f.write(a.tobytes())


def read_range_output(path, n, c):
    """what lift_range_check wrote -> (coeffs [n,c], recon [n,c], lcp int8[32])"""
    raw = np.fromfile(path, dtype=np.uint8)
    co = raw[:4 * n * c].view(np.int32).reshape(n, c)
    rec = raw[4 * n * c:8 * n * c].view(np.int32).reshape(n, c)
    lcp = raw[8 * n * c:8 * n * c + 32].view(np.int8)
    return co, rec, lcp


def build_range_check(out_dir):
    """gcc: tests/lift_range_check.c + oracle/lift_oracle.c with the signed-overflow sanitizer, a
    stand-alone program -> its path"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(out_dir, "lift_range_check")
    subprocess.run(["gcc", "-O1", "-std=c11", "-fsanitize=signed-integer-overflow", "-fno-sanitize-recover=all",
                    "-I", os.path.join(root, "include"), "-I", os.path.join(root, "oracle"),
                    os.path.join(root, "tests", "lift_range_check.c"), os.path.join(root, "oracle", "lift_oracle.c"),
                    "-o", exe, "-lm"], check=True)
    return exe
