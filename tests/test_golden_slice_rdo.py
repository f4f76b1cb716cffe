"""tests/golden/slice_rdo_golden.npz -- the compiled reference's slice-level inter / intra decisions -- is
self-consistent, covers what it has to, and its generator is reproducible where the reference tree is present."""
import os
import subprocess
import sys

import numpy as np
import pytest

import slice_rdo_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("GPCC_REFERENCE", "/root/reference")


def test_fixture_lists_the_cases():
    g = sc.golden()
    assert list(g["names"]) == sc.NAMES
    assert os.path.getsize(sc.GOLDEN) < 256 * 1024


@pytest.mark.parametrize("name", sc.NAMES)
def test_decision_follows_from_the_stored_figures(name):
    c = sc.case(name)
    q = int(c["init_qp_minus4"] / 3)
    lam = (0.85 * 2.0 ** q) ** 0.5
    cost = [float(c["dist"][k]) + lam * int(c["bytes"][k]) for k in (0, 1)]
    assert (cost[0] > cost[1]) == c["intra_wins"]
    assert np.array_equal(sc.golden()[name + "/cost"], np.array(cost))
    assert c["init_qp_minus4"] == sc.CASES[name]["layers"][0] - 4
    inp = sc.inputs(name)
    assert (len(inp["xyz"]), len(inp["xyz_ref"])) == (c["n"], c["n_ref"]), "the seeded clouds have changed"


def test_coverage():
    wins = {(sc.CASES[n]["transform"], sc.case(n)["intra_wins"]) for n in sc.NAMES}
    assert wins == {(1, False), (1, True), (2, False), (2, True)}, "both outcomes for both transforms"
    qs = {sc.case(n)["init_qp_minus4"] % 3 for n in sc.NAMES}
    assert {0, 2} <= qs, "init_qp_minus4 on both sides of a multiple of 3"
    assert len({sc.CASES[n]["search_range"] for n in sc.NAMES}) >= 2
    assert any(len(sc.CASES[n]["layers"]) > 1 for n in sc.NAMES)
    assert any(sc.CASES[n].get("cached_dist2_delta") for n in sc.NAMES)
    # at least one case per transform where the costs are within 12 %
    for t in (1, 2):
        close = [abs(c[0] - c[1]) / max(c) for n in sc.NAMES if sc.CASES[n]["transform"] == t
                 for c in [sc.golden()[n + "/cost"]]]
        assert min(close) < 0.12, (t, close)


def test_tiny_cases_are_stored_in_full():
    g = sc.golden()
    for name in sc.FULL:
        assert sc.digest(g[name + "/payload"], np.uint8) == sc.case(name)["payload_sha"]
        assert sc.digest(g[name + "/recon"].astype(np.int32)) == sc.case(name)["recon_sha"]
        assert len(g[name + "/recon"]) == sc.case(name)["n"]


def test_generator_is_reproducible(tmp_path):
    if not (os.path.isdir(os.path.join(REF, "tmc3"))
            and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libtmc3_ref.so"))):
        pytest.skip("the reference tree / oracle/_ref/libtmc3_ref.so is not here")
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_slice_rdo_golden", os.path.join(ROOT, "tests", "golden", "make_slice_rdo_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    lib = gen.build_harness(str(tmp_path))
    for name in ("lift_tiny", "pred_tiny", "lift_qp_at3", "pred_cached_delta"):
        inp = sc.inputs(name)
        on = gen.run_case(lib, inp, rdo=True)
        c = sc.case(name)
        assert (on["inter_after"] == 0) == c["intra_wins"]
        assert sc.digest(np.frombuffer(on["payload"], np.uint8), np.uint8) == c["payload_sha"]
        assert sc.digest(on["recon"]) == c["recon_sha"]
        assert (int(on["dist_after"]), on["rate_after"]) == (int(c["dist"][1]), int(c["bytes"][1]))
