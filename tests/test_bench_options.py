"""bench.py's plain / --full split, --dump-outputs (benchlib/outputs.py) and the wall budget of the --full legs: CPU only."""
import importlib.util
import json
import os
import subprocess
import time

import numpy as np

import conftest
from benchlib import legs, outputs


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(conftest.ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plain_run_is_the_default_and_full_is_an_option():
    b = _bench_module()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = b.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_kept_rows_all_when_they_fit_else_a_fixed_seeded_sample():
    assert np.array_equal(outputs.kept_rows(100, 10, budget=1000), np.arange(100))
    r = outputs.kept_rows(1000, 10, budget=2000)
    assert r.size == 200 and np.array_equal(r, np.unique(r)) and r.min() >= 0 and r.max() < 1000
    assert np.array_equal(r, outputs.kept_rows(1000, 10, budget=2000)), "the sample must not change from run to run"


def test_default_workloads_fit_the_budget():
    """c3 (32 x 1024^2) and c4 (one 3840x2160 image): stereo pair + uint16 depth + normal map, float32, under 64 MB."""
    for n, h, w in ((32, 1024, 1024), (1, 2160, 3840), (8, 1080, 1920)):
        row_bytes = 4 * (2 * w * 3 + w + w * 3)
        kept = outputs.kept_rows(n * h, row_bytes).size
        assert 0 < kept <= n * h and kept * row_bytes + 3 * 256 < 64 * 10 ** 6


def test_dump_outputs_same_rows_for_every_output(tmp_path):
    rng = np.random.default_rng(3)
    n, h, w = 3, 40, 24
    sbs = rng.integers(0, 256, (n, h, 2 * w, 3), dtype=np.uint8)
    d16 = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    f64 = rng.normal(size=(n, h, w))
    row_bytes = 4 * (2 * w * 3 + w) + 8 * w
    budget = 50 * row_bytes
    man = outputs.dump_outputs(str(tmp_path), {"stereo_pair": sbs, "depth_u16": d16, "normal_map": None, "extra": f64}, budget=budget)
    assert sorted(os.listdir(tmp_path)) == ["depth_u16.npy", "extra.npy", "manifest.json", "stereo_pair.npy"]
    rows = np.array(man["rows"])
    assert rows.size == 50 and man["rows_total"] == n * h
    assert json.load(open(tmp_path / "manifest.json"))["rows"] == man["rows"]
    got_s, got_d, got_f = (np.load(tmp_path / f) for f in ("stereo_pair.npy", "depth_u16.npy", "extra.npy"))
    assert got_s.dtype == np.float32 and got_d.dtype == np.float32 and got_f.dtype == np.float64
    assert np.array_equal(got_s, sbs.reshape(n * h, 2 * w, 3)[rows].astype(np.float32))
    assert np.array_equal(got_d, d16.reshape(n * h, w)[rows].astype(np.float32))
    assert np.array_equal(got_f, f64.reshape(n * h, w)[rows])
    assert sum(os.path.getsize(tmp_path / f) for f in ("stereo_pair.npy", "depth_u16.npy", "extra.npy")) <= budget + 3 * 256


def test_dump_outputs_whole_arrays_when_small(tmp_path):
    d16 = np.arange(2 * 5 * 7, dtype=np.uint16).reshape(2, 5, 7)
    man = outputs.dump_outputs(str(tmp_path), {"depth_u16": d16})
    assert man["rows"] is None and man["sample"] is None
    assert np.array_equal(np.load(tmp_path / "depth_u16.npy"), d16.reshape(10, 7).astype(np.float32))


def test_full_legs_start_nothing_once_the_wall_budget_is_spent(monkeypatch):
    def no_run(*a, **k):
        raise AssertionError("a leg was started after the deadline")
    monkeypatch.setattr(legs.subprocess, "run", no_run)
    out = legs.other_configs_leg(240.0, deadline=time.perf_counter() - 1.0)
    assert set(out) == {"c5", "c2", "c3match", "c4", "c4_rmax3000"}
    assert all(v["error"].startswith("not run") for v in out.values())


def test_full_legs_stop_after_a_failed_leg(monkeypatch):
    calls = []

    def failing_run(cmd, **k):
        calls.append(cmd)
        assert "--full" in cmd and k["timeout"] <= 240.0
        return subprocess.CompletedProcess(cmd, 134, stdout="", stderr="aborted")
    monkeypatch.setattr(legs.subprocess, "run", failing_run)
    out = legs.other_configs_leg(240.0, deadline=time.perf_counter() + 1000.0)
    assert len(calls) == 1 and out["c5"]["error"] == "exit code 134"
    assert all(out[k]["error"] == "not run: leg c5 failed" for k in ("c2", "c3match", "c4", "c4_rmax3000"))
