"""Case table of the predicting transform's edge tests (TEST INFRASTRUCTURE): what
tests/golden/make_pred_edges_golden.py stores in pred_edges_golden.npz and what
tests/test_oracle_pred_edges.py / tests/test_gpu_pred_edges.py walk.

Geometries: two small random clouds (six levels of detail; ten, the last four of equal size, on
which the running `quantLayer` / `lod` counters stall) and 700 lidar points as ONE level (a deep
DAG that spans eleven 64-predictor claims).  The LoD structures are the reference's
(AttributeLods::generate, predicting CTC parameters: intra-LoD prediction over the whole range,
no skipped layers, weight blending for colour).

Fields, per bit depth: full-range random values; 0 / max at random (the largest residuals: both
clips of the write-back at a lossy QP, near-ties among the direct predictors at a low one); max
with probability 0.1; all max (nothing eligible, every sum of the coefficient estimation zero);
values whose neighbour spread sits on both sides of the eligibility threshold `64 << (bd - 8)`;
and components built to drive the inter-component coefficients to 8 and to 0.

Parameter sets: QP at and beyond both clamps, chroma offsets that clamp the second quantiser, one
QP region that reaches both clamps per point; and the tools (number of direct predictors, the
average predictor, thresholds 0 and 255, quant_neigh_weight sums 255 / 256 on either side of the
packed share word, the whole share on the first neighbour).

The reference's coder buffer holds 6 n + 1024 bytes and the process aborts beyond it: full-range
16-bit colour passes it at QP 4 and at QP 8, so that field is coded from QP 22 upwards (no case of
the table was dropped for it; the field simply has no qp4 / chroma_lo set)."""
import os

import numpy as np

import lift_edge_cases as lec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pred_edges_golden.npz")

FixtureWriter, Fixture, i32, max_qp = lec.FixtureWriter, lec.Fixture, lec.i32, lec.max_qp

GEOM = {"r1500": dict(kind="random", n=1500, seed=5, bits=5, levels=12),    # six levels
        "r300": dict(kind="random", n=300, seed=5, bits=9, levels=12),      # ten, the last four of equal size
        "l700": dict(kind="lidar", n=700, seed=71, levels=1)}               # one level: a deep DAG
NPL = {"r1500": [1, 8, 62, 341, 960, 1500], "r300": 10, "l700": [700]}

# one QP region: origin, size (the reference's box is inclusive at origin + size)
REGION_BOX = ((0, 0, 0), (16, 32, 32))


def positions(geom):
    from mpeg_pcc_tmc13_amd import synth
    g = GEOM[geom]
    if g["kind"] == "random":
        return synth.random_cloud(n=g["n"], seed=g["seed"], bits=g["bits"])[0]
    xyz = synth.lidar_cloud(g["n"], seed=g["seed"])[0][:g["n"]]
    assert len(xyz) == g["n"]
    return np.ascontiguousarray(xyz)


def lod_parameters(geom, c):
    """predicting CTC: transformType 1, both search ranges 1100000, no skipped layers, blending for colour"""
    from mpeg_pcc_tmc13_amd import lod_params
    lp = lod_params(levels=GEOM[geom]["levels"], lifting=False, intra_range=1100000, blend=(c == 3))
    lp.intra_lod_prediction_skip_layers = 0
    return lp


def threshold_of(bd, raw=64):
    return raw << (bd - 8)


def field_attrs(geom, kind, c, bd):
    """int32 [n, c]"""
    n = GEOM[geom]["n"]
    top = (1 << bd) - 1
    if kind == "rand":
        a = np.random.default_rng(10).integers(0, 1 << bd, size=(n, c))
    elif kind == "bin":
        a = np.where(np.random.default_rng(11).random((n, c)) < 0.5, 0, top)
    elif kind == "bin10":
        a = np.where(np.random.default_rng(15).random((n, c)) < 0.1, top, 0)
    elif kind == "const":
        a = np.full((n, c), top)
    elif kind == "thr":
        t = threshold_of(bd)
        a = (1 << (bd - 1)) + np.array([0, t - 1, t, t + 1])[np.random.default_rng(16).integers(0, 4, size=(n, c))]
    else:
        assert kind == "icp" and c == 3
        g = np.random.default_rng(17).integers(0, top // 4, size=n)
        a = np.stack([g, np.minimum(top, 2 * g), top - 2 * g], axis=1)
    assert a.min() >= 0 and a.max() <= top
    return np.ascontiguousarray(a, dtype=np.int32)


def param_sets(bd):
    """-> {set name: (qp, chroma offset, region offsets or None)}"""
    mq = max_qp(bd)
    return {"qp4": (4, 0, None),                       # lower bound
            "qp6": (6, 0, None),
            "qp10": (10, 0, None),
            "qp22": (22, 0, None),
            "qp34": (34, 0, None),
            "qpmax": (mq, 0, None),                    # upper bound
            "qpmax20": (mq + 20, 0, None),             # above the upper clamp
            "chroma_lo": (8, -20, None),               # second quantiser clamped low
            "chroma_hi": (mq - 2, 20, None),           # second quantiser clamped high
            "region_lo": (6, -1, (-20, -20)),          # both quantisers clamped low inside the box
            "region_hi": (mq - 3, 1, (20, 20))}        # ... and high


TIES = {"tie_bd12_qp4": (12, 4), "tie_bd14_qp5": (14, 5), "tie_bd16_qp10": (16, 10)}


def _table():
    """-> [(name, geom, field kind, c, bd, set name, tool overrides)]"""
    t = []

    def add(geom, kind, c, bd, sets, **tools):
        for s in sets:
            t.append((geom, kind, c, bd, s, tools))

    # ---- r1500 ----
    for bd in (8, 10, 12):
        add("r1500", "rand", 3, bd, ("qp4", "qpmax", "qpmax20", "chroma_lo", "chroma_hi"))
    add("r1500", "rand", 3, 16, ("qp34", "qp22", "qpmax", "qpmax20", "chroma_hi"))    # (the coder buffer, above)
    for bd in (8, 12, 16):
        add("r1500", "rand", 1, bd, ("qp4", "qpmax20"))
        add("r1500", "bin", 3, bd, ("qp4", "qpmax", "qpmax20", "chroma_lo", "chroma_hi", "region_lo", "region_hi"))
        add("r1500", "bin10", 3, bd, ("qp4", "qpmax"))
        add("r1500", "const", 3, bd, ("qp4", "qpmax"))
        add("r1500", "thr", 3, bd, ("qp4", "qp22"))
        add("r1500", "thr", 1, bd, ("qp4",))
        add("r1500", "icp", 3, bd, ("qp10" if bd == 16 else "qp4", "qp34"))
        add("r1500", "icp", 3, bd, ("qp10" if bd == 16 else "qp4", "qp34"), icp=False)
    for bd in (8, 16):
        add("r1500", "bin", 1, bd, ("qp4", "qpmax", "region_lo", "region_hi"))
    add("r1500", "bin10", 1, 16, ("qp4",))
    add("r1500", "const", 1, 8, ("qp4",))
    # quant_neigh_weight: sum 255 (the packed share word) and 256 (the wide path); at a QP whose step exceeds one,
    # below which min(weight, step) >> 8 is 1 whatever the weights are
    for qnw in ((85, 85, 85), (86, 85, 85)):
        add("r1500", "bin", 3, 8, ("qp34",), quant_neigh_weight=qnw)
        add("r1500", "rand", 1, 16, ("qp34",), quant_neigh_weight=qnw)
    # the regression cases of the rate sum's order
    for name, (bd, qp) in TIES.items():
        t.append(("r1500", "bin", 3, bd, name, {}))
    # ---- r300: the level counters stall on the last four levels ----
    add("r300", "rand", 3, 8, ("qp4", "qpmax20"))
    add("r300", "rand", 3, 16, ("qp34", "qpmax20"))
    add("r300", "rand", 1, 16, ("qp4", "qpmax20"))
    add("r300", "bin", 3, 12, ("qp4", "qpmax", "chroma_lo", "chroma_hi"))
    add("r300", "const", 3, 8, ("qp4",))
    add("r300", "icp", 3, 8, ("qp4",))
    add("r300", "thr", 3, 12, ("qp4",))
    for direct in (0, 1, 2, 3):
        for avg_disabled in (False, True):
            if direct == 0 and avg_disabled:
                continue
            add("r300", "bin", 3, 12, ("qp6",), direct=direct, avg_disabled=avg_disabled)
            add("r300", "bin", 1, 16, ("qp6",), direct=direct, avg_disabled=avg_disabled)
    add("r300", "thr", 3, 12, ("qp6",), threshold=0)
    add("r300", "bin", 3, 8, ("qp6",), threshold=255)
    add("r300", "bin", 3, 12, ("qp6",), threshold=255)
    # ---- l700: one level, lane-to-lane hand-over and granule polls ----
    for bd in (8, 16):
        add("l700", "rand", 1, bd, ("qp4", "qpmax"), avg_disabled=True)
    add("l700", "bin", 1, 16, ("qp4", "qpmax"), avg_disabled=True)
    add("l700", "thr", 1, 16, ("qp4",), avg_disabled=True)
    add("l700", "bin", 3, 8, ("qp4",))
    add("l700", "rand", 3, 12, ("qp4",))
    add("l700", "bin", 1, 16, ("qp34",), avg_disabled=True, quant_neigh_weight=(255, 0, 0))
    add("l700", "bin", 3, 8, ("qp34",), avg_disabled=True, quant_neigh_weight=(255, 0, 0))
    return t


def tool_tag(tools):
    """the part of a case's name that states its tools"""
    parts = []
    if "direct" in tools or "avg_disabled" in tools:
        parts.append(f"d{tools.get('direct', 3)}a{int(tools.get('avg_disabled', False))}")
    if "threshold" in tools:
        parts.append(f"thr{tools['threshold']}")
    if "icp" in tools:
        parts.append("noicp")
    if "quant_neigh_weight" in tools:
        parts.append("qnw" + "_".join(str(v) for v in tools["quant_neigh_weight"]))
    return "+".join(parts)


def cases():
    """-> [dict(name, geom, kind, c, bd, field (its fixture key), pk (pred_params keywords), region (the per-region
    offsets or None))] -- the whole table, in the fixture's order"""
    out, seen = [], set()
    for geom, kind, c, bd, sname, tools in _table():
        if sname in TIES:
            qp, chroma, region = TIES[sname][1], 0, None
            name = sname
        else:
            qp, chroma, region = param_sets(bd)[sname]
            tag = tool_tag(tools)
            name = f"{geom}/{kind}_bd{bd}_c{c}/{sname}" + (f"/{tag}" if tag else "")
        assert name not in seen, name
        seen.add(name)
        pk = dict(qp=qp, chroma_offset=chroma, bitdepth=bd, direct=3, avg_disabled=False, threshold=64, icp=True,
                  quant_neigh_weight=(0, 0, 0), max_levels=GEOM[geom]["levels"])
        pk.update(tools)
        out.append(dict(name=name, geom=geom, kind=kind, c=c, bd=bd, field=f"field/{geom}/{kind}_bd{bd}_c{c}", pk=pk,
                        set=sname, region=region))
    return out


def regions_of(case):
    """the case's QP regions as params.set_qp_regions / params.region_offsets take them"""
    lo, size = REGION_BOX
    return [(lo, tuple(a + b for a, b in zip(lo, size)), case["region"])]


def qp_offsets(case, xyz):
    """per-point (luma, chroma) offsets [n, 2] of a region case, None otherwise"""
    from mpeg_pcc_tmc13_amd.params import region_offsets
    return None if case["region"] is None else region_offsets(xyz, regions_of(case))


def pred_parameters(case, npl):
    from mpeg_pcc_tmc13_amd import pred_params
    return pred_params(npl, **case["pk"])


def effective_qps(pp, indexes, qp_off):
    """(qp of the first, of the second quantiser) per predictor of QP layer 0, before and after the clamps
    -> (raw0, qp0, raw1, qp1)"""
    n = len(indexes)
    o = np.zeros((n, 2), np.int64) if qp_off is None else np.asarray(qp_off, np.int64)[np.asarray(indexes)]
    raw0 = int(pp.layer_qp[0][0]) + o[:, 0]
    qp0 = np.clip(raw0, 4, pp.max_qp)
    raw1 = int(pp.layer_qp[0][1]) + o[:, 1] + qp0
    qp1 = np.clip(raw1, 4, pp.max_qp)
    return raw0, qp0, raw1, qp1


def neighbour_spread(lod, rec):
    """per predictor the largest spread of a component among its neighbours' reconstructions (what
    predModeEligible* compares with the threshold); -1 where there are fewer than two neighbours.
    rec [n, c] in point order"""
    coded = np.asarray(rec, np.int64)[np.asarray(lod["indexes"])]
    nc, ni = np.asarray(lod["nc"]), np.asarray(lod["ni"])
    nb = coded[ni]                                                   # [n, 3, c]
    used = np.arange(3)[None, :, None] < nc[:, None, None]
    hi = np.where(used, nb, -1).max(axis=1)
    lo = np.where(used, nb, 1 << 40).min(axis=1)
    return np.where(nc > 1, (hi - lo).max(axis=1), -1)


def structure(g, geom, c):
    return lec.structure(g, f"geom/{geom}/c{c}")


def fixture_cases(g):
    """-> [(case, pred params, LoD structure, attrs, qp_off or None)] for every case of the table, from the fixture"""
    out = []
    for case in cases():
        lod = structure(g, case["geom"], case["c"])
        q = g[f"geom/{case['geom']}/{case['set']}"] if case["region"] is not None else None
        out.append((case, pred_parameters(case, lod["npl"]), lod, g[case["field"]], q))
    return out


def stored(g, case):
    """-> (values [n,c] coding order, reconstruction [n,c] point order, icp int8 [32,3], sha256 of the coded payload)"""
    import ast
    key = "case/" + case["name"]
    rec = ast.literal_eval(g.params[key])
    return g[key + "/values"], g[key + "/rec"], g[key + "/icp"].astype(np.int8), rec["sha"]
