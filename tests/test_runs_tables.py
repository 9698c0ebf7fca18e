"""binding.flatten_runs: the flat tables of the run entries (lk_batch_replay_overlay_runs_dev, lk_batch_replay_runs_dev) from nested host inputs -
offsets, dtypes, message counts, an empty message array in the middle.  No GPU, no library."""
import numpy as np
import pytest

from legkilo_amd import binding, synth


def scan(n, first):
    pts = np.zeros(n, dtype=synth.POINT_DTYPE)
    pts["x"] = first + np.arange(n)
    pts["curvature"] = np.linspace(0.0, 0.09, n, dtype=np.float32)
    return pts


def imu(n, t0):
    m = np.zeros(n, dtype=synth.IMU_DTYPE)
    m["stamp"] = t0 + 0.001 * np.arange(n)
    return m


RUNS = [[scan(3, 0), scan(1, 100)], [scan(5, 200)], [scan(2, 300), scan(4, 400), scan(1, 500)]]
TBS = [[1.0, 1.1], [2.0], [3.0, 3.1, 3.2]]


def test_offsets_and_dtypes_without_messages():
    t = binding.flatten_runs(RUNS, TBS)
    assert t["run_off"].dtype == np.uint32 and t["run_off"].tolist() == [0, 2, 3, 6]
    assert t["scan_off"].dtype == np.uint64 and t["scan_off"].tolist() == [0, 3, 4, 9, 11, 15, 16]
    assert t["t_begin"].dtype == np.float64 and t["t_begin"].tolist() == [1.0, 1.1, 2.0, 3.0, 3.1, 3.2]
    assert t["pts"].dtype == synth.POINT_DTYPE and t["pts"].flags["C_CONTIGUOUS"] and t["pts"].itemsize == 16
    assert t["pts"]["x"].tolist() == [0, 1, 2, 100, 200, 201, 202, 203, 204, 300, 301, 400, 401, 402, 403, 500]
    assert t["msg_kind"] == 0 and t["n_msg"] is None and t["msgs"] is None


def test_message_counts_with_an_empty_array_in_the_middle():
    imus = [[imu(2, 1.0), imu(0, 1.1)], [imu(3, 2.0)], [imu(0, 3.0), imu(1, 3.1), imu(0, 3.2)]]
    t = binding.flatten_runs(RUNS, TBS, imus=imus)
    assert t["msg_kind"] == 1
    assert t["n_msg"].dtype == np.uint32 and t["n_msg"].tolist() == [2, 0, 3, 0, 1, 0]
    assert t["msgs"].dtype == synth.IMU_DTYPE and t["msgs"].itemsize == 56 and t["msgs"].flags["C_CONTIGUOUS"]
    assert np.allclose(t["msgs"]["stamp"], [1.0, 1.001, 2.0, 2.001, 2.002, 3.1])
    # scan s's records are msgs[off[s] : off[s + 1]] with off the prefix sum of n_msg
    off = np.r_[0, np.cumsum(t["n_msg"])]
    per_scan = [m for run in imus for m in run]
    for s, m in enumerate(per_scan):
        assert np.array_equal(t["msgs"][off[s]:off[s + 1]], m)


def test_kin_records_and_no_records_at_all():
    kins = [[np.zeros(1, dtype=synth.KIN_DTYPE), np.zeros(0, dtype=synth.KIN_DTYPE)], [np.zeros(2, dtype=synth.KIN_DTYPE)],
            [np.zeros(0, dtype=synth.KIN_DTYPE)] * 3]
    t = binding.flatten_runs(RUNS, TBS, kins=kins)
    assert t["msg_kind"] == 2 and t["n_msg"].tolist() == [1, 0, 2, 0, 0, 0] and t["msgs"].itemsize == 264 and len(t["msgs"]) == 3
    none = binding.flatten_runs(RUNS, TBS, imus=[[imu(0, 0.0)] * len(run) for run in RUNS])
    assert none["msg_kind"] == 1 and none["n_msg"].tolist() == [0] * 6 and none["msgs"] is None


def test_nesting_must_agree():
    with pytest.raises(AssertionError):
        binding.flatten_runs(RUNS, [[1.0, 1.1], [2.0], [3.0, 3.1]])
    with pytest.raises(AssertionError):
        binding.flatten_runs(RUNS, TBS, imus=[[imu(1, 1.0)]])
    with pytest.raises(AssertionError):
        binding.flatten_runs(RUNS, TBS, imus=[], kins=[])
