"""bench.py's two modes on a small batch: a plain run does only what its headline needs (no extra, no checker), `--full` still runs
every extra and its in-line parity check against the oracle."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--scans-per-gpu", "32", "--map-warm", "4", "--steps", "2", "--warmup", "1"]
EXTRA_PREFIXES = ("sustained_", "shard128_", "shuffled_", "overlay_", "config1_", "config2_", "config4_", "stream", "pcie_", "state_record")


def run_bench(args, timeout_s):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout_s)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_only(tmp_path):
    line = run_bench(["--dump-outputs", str(tmp_path / "dump")], 300)
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "scans/s" and line["dtype"] == "f64"
    assert line["cpu_baseline"] is None and line["parity_check"] is None
    assert line["extra"]["full"] is False
    assert [k for k in line["extra"] if k.startswith(EXTRA_PREFIXES)] == []
    assert "launch_ms_single_stream_events" not in line["roofline"]
    assert os.path.exists(tmp_path / "dump" / "pose_pos.npy")


@pytest.mark.gpu
def test_full_run_keeps_every_extra_and_the_parity_check():
    line = run_bench(["--full", "--cpu-sample", "8", "--stream-scans", "3", "--overlay-scans", "32", "--overlay-check", "4", "--config1-scans", "64",
                      "--config2-scans", "4", "--config2-check", "1", "--config4-scans", "3", "--shuffle-check", "4", "--sustained-s", "0.05"], 600)
    e = line["extra"]
    assert e["full"] is True
    for k in ("sustained_scans_per_s", "shuffled_in_bucket_ms_per_step", "overlay_scans_per_s", "config1_ragged_scans_per_s", "config2_scans_per_s",
              "config4_path_ms_per_scan", "stream_scans_per_s", "pcie_inclusive_ms_per_step", "state_records_gathered"):
        assert k in e, k
    assert "launch_ms_single_stream_events" in line["roofline"]
    assert line["cpu_baseline"]["value"] > 0
    p = line["parity_check"]
    assert p["ok"] and p["n"] == 8 and {"overlay", "config2_rows", "config1_ragged", "config4_live", "shuffled_in_bucket"} <= set(p), p
