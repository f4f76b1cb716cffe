"""bench.py --dump-outputs: the files hold what the last timed step computed (here: what the CPU oracle computes for the
same seeded frame), as float64, within the size budget; an output over its share is cut to the same sample every time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_within_budget_and_sample_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * (128 + 8 * 1000))
    small = torch.arange(-500, 500, dtype=torch.int32)          # exactly its share: written whole
    big = torch.arange(5000, dtype=torch.int32) * 400_000        # beyond float32's integers
    tensors = {"small": small, "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), tensors)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in tensors}
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["small"], small.numpy())
    # the sample: 1000 distinct elements of `big`, in index order, every value exact
    assert a["big"].shape == (1000,) and np.all(np.diff(a["big"]) > 0)
    assert np.all(np.isin(a["big"].astype(np.int64), big.numpy().astype(np.int64)))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BUDGET_BYTES
    for k in tensors:
        assert np.array_equal(a[k], np.load(tmp_path / "b" / (k + ".npy")))


@pytest.mark.gpu
def test_dumped_outputs_are_the_oracles(tmp_path):
    import oracle_loader as ol
    from mpeg_pcc_tmc13_amd import raht_params
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--points", "60000", "--no-extras", "--no-profile", "--no-cpu-baseline", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert line["steps"] == 2 and line["config"]["roundtrip_decoder_equals_encoder_recon"] is True
    morton, attrs, _ = bench.make_frame("lidar", 60000, seed=1)
    co, rec = ol.oracle().raht_forward(raht_params(qp=34, subnode=True, search_range=2500), morton, attrs)
    got = {k: np.load(os.path.join(out, k + ".npy")) for k in ("coefficients", "reconstruction", "decoded")}
    assert sorted(os.listdir(out)) == ["coefficients.npy", "decoded.npy", "reconstruction.npy"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["coefficients"], co)
    assert np.array_equal(got["reconstruction"], rec.reshape(-1))
    assert np.array_equal(got["decoded"], rec.reshape(-1))
