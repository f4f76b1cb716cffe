"""bench.py without --full is the headline alone: set-up, warm-up, the timed steps, the line.  Everything measured or
checked beside it -- roofline, extra legs, CPU baselines -- runs with --full, and the options that shape those need it."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config"}


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_every_extra_off(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "4", "--warmup", "2")
    assert not a.full and a.no_extras and a.no_profile and a.no_cpu_baseline and not a.verify_gather
    assert (a.steps, a.warmup, a.points, a.frames, a.direction) == (4, 2, 1_000_000, 1, "both")


def test_full_runs_everything_and_its_options_take_parts_away(monkeypatch):
    a = parse(monkeypatch, "--full")
    assert a.full and not (a.no_extras or a.no_profile or a.no_cpu_baseline) and a.verify_gather
    a = parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-extras", "--legs", "lifting")
    assert a.no_cpu_baseline and a.no_extras and not a.no_profile and a.legs == "lifting"


def test_legs_without_full_is_an_error(monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        parse(monkeypatch, "--legs", "lifting")
    assert e.value.code == 2 and "--full" in capsys.readouterr().err


@pytest.mark.gpu
def test_plain_line_has_the_headline_and_nothing_else():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--points", "60000"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert set(d) == HEADLINE_KEYS
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert set(d["config"]) == {"workload", "points_per_gpu_per_step", "frames_per_gpu",
                                "roundtrip_decoder_equals_encoder_recon"}
    assert d["config"]["roundtrip_decoder_equals_encoder_recon"] is True
