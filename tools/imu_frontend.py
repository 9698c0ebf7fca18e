"""Time of the IMU front end and of the first frame on the device.

  - lk_decode_imu_dev + lk_imu_split_dev on a recorded-run-sized input - 1 024 scans x 20 sensor_msgs/Imu messages (200 Hz against 10 Hz scans),
    frame_id lengths 0 .. 40 mixed per message, every message kept - in steady state after warm-up, between HIP events on the handle's stream,
    next to the numpy restatement's CPU time (tests/imu_ref.py, tests/kin_ref.py) for the same work;
  - lk_first_frame_dev on a VLP-16-shaped raw cloud (28 800 rays) with the 20 records of its package, next to the start composed on the host
    (running mean and cloudLidarToWorld in numpy, lk_set_state + lk_init_process_cov_q + lk_map_build), wall clock, each on a fresh map.

    python tools/imu_frontend.py [--iters 50] [--warmup 5]

Prints one JSON line.  The entries are synchronous (each reads back a few words), so the event intervals include their host round trips."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lk_pkg  # noqa: E402

lk_pkg.load()
import imu_ref  # noqa: E402
import kin_ref  # noqa: E402
import scenes  # noqa: E402
from legkilo_amd import binding, config, synth  # noqa: E402

REC = synth.IMU_DTYPE.itemsize


def front_end(a, hip, P):
    n = a.scans * a.per_scan
    t0 = 2.0
    imus = synth.imu_stream(synth.Trajectory(), t0, t0 + n / 200.0, seed=123)
    assert len(imus) == n
    rng = np.random.default_rng(5)
    buf, off = synth.imu_messages(imus, [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(0, 41, n)], seed=6)
    ends = t0 + (np.arange(a.scans) + 1) * (a.per_scan / 200.0) - 4e-3   # between two messages; the newest message lies beyond the last end
    g = binding.LegKiloHip(config.make_config(P, max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12))
    d_msgs, d_imus = g.device_malloc(buf.nbytes), g.device_malloc(n * REC)
    g.h2d(d_msgs, buf)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    stream = C.c_void_p(g.stream())
    dec_ms, split_ms, wall_ms = [], [], []
    ms = C.c_float()
    for it in range(a.warmup + a.iters):
        g.imu_configure(True)   # host-side reset: every iteration decodes the same stream from the start
        w0 = time.perf_counter()
        hip.hipEventRecord(ev[0], stream)
        k = g.decode_imu_dev(d_msgs, off, d_imus)
        hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        d_ms = ms.value
        hip.hipEventRecord(ev[0], stream)
        n_msg, npk, ncs = g.imu_split_dev(d_imus, k, ends)
        hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        w1 = time.perf_counter()
        if it >= a.warmup:
            dec_ms.append(d_ms)
            split_ms.append(ms.value)
            wall_ms.append((w1 - w0) * 1e3)
    assert k == n and npk == a.scans and ncs == n - 1, (k, npk, ncs)
    c0 = time.perf_counter()
    ref = imu_ref.Frontend(True).process(buf, off)
    kin_ref.sync_package(ref["stamp"], ends)
    cpu_ms = (time.perf_counter() - c0) * 1e3
    recs = np.zeros(k, dtype=synth.IMU_DTYPE)
    g.d2h(recs, d_imus)
    same = recs.tobytes() == ref.tobytes()
    g.device_free(d_msgs)
    g.device_free(d_imus)
    g.close()
    for e in ev:
        hip.hipEventDestroy(e)
    med = lambda v: float(np.median(v))  # noqa: E731
    return dict(messages=n, scans=a.scans, bytes=int(buf.nbytes), kept=int(k), iters=a.iters, decode_ms_median=round(med(dec_ms), 4),
                decode_ms_min=round(min(dec_ms), 4), split_ms_median=round(med(split_ms), 4), split_ms_min=round(min(split_ms), 4),
                wall_ms_median=round(med(wall_ms), 4), numpy_restatement_ms=round(cpu_ms, 1), records_match_restatement=bool(same))


def first_frame(a, P):
    sc = scenes.Scene(params=P, max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
    t0 = 2.0
    raw = synth.vlp16_scan(sc.world, scenes.Frozen(sc.traj, t0), t0, P)
    imus = synth.imu_stream(sc.traj, t0 - 0.1, t0, seed=77)
    E, T = np.array(P["extrinsic_R"], float).reshape(3, 3), np.array(P["extrinsic_T"], float)
    dev_ms, host_ms = [], []
    state = {}
    for it in range(a.warmup + a.ff_iters):
        for mode in ("dev", "host"):
            g = binding.LegKiloHip(sc.cfg())   # BuildVoxelMap runs once per map: a fresh handle per start
            d_raw, d_imus = g.device_malloc(raw.nbytes), g.device_malloc(imus.nbytes)
            g.h2d(d_raw, raw)
            g.h2d(d_imus, imus)
            g.synchronize()
            w0 = time.perf_counter()
            if mode == "dev":
                g.first_frame_dev(d_raw, len(raw), t0, 1, d_imus, len(imus))
            else:   # what a caller did before: both arrays back to the host, the start composed there
                pts, rec = np.zeros(len(raw), dtype=synth.POINT_DTYPE), np.zeros(len(imus), dtype=synth.IMU_DTYPE)
                g.d2h(pts, d_raw)
                g.d2h(rec, d_imus)
                mean = np.r_[rec["acc"][0], rec["gyr"][0]]
                for k in range(len(rec)):
                    mean = mean + (np.r_[rec["acc"][k], rec["gyr"][k]] - mean) / (k + 1.0)
                norm = float(np.sqrt(mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2]))
                x = np.zeros(36)
                x[[0, 4, 8]] = 1.0
                x[18:21], x[21:24] = mean[3:], (-mean[:3]) / norm * P["gravity"]
                g.set_state(x, 1e-6 * np.eye(30))
                g.init_process_cov_q()
                g.set_acc_norm(norm)
                g.set_times(t0, t0)
                xb = scenes.xyz_of(pts)
                g.map_build(((xb.astype(np.float64) @ E.T + T) @ x[:9].reshape(3, 3).T + x[9:12]).astype(np.float32), xb)
            w1 = time.perf_counter()
            state[mode] = (g.get_state()[0], g.get_acc_norm(), g.map_stats())
            g.device_free(d_raw)
            g.device_free(d_imus)
            g.close()
            if it >= a.warmup:
                (dev_ms if mode == "dev" else host_ms).append((w1 - w0) * 1e3)
    same = bool(np.array_equal(state["dev"][0], state["host"][0]) and state["dev"][1:] == state["host"][1:])
    med = lambda v: float(np.median(v))  # noqa: E731
    return dict(first_frame_points=len(raw), first_frame_messages=len(imus), first_frame_iters=a.ff_iters,
                first_frame_dev_ms_median=round(med(dev_ms), 3), first_frame_dev_ms_min=round(min(dev_ms), 3),
                first_frame_host_composed_ms_median=round(med(host_ms), 3), first_frame_host_composed_ms_min=round(min(host_ms), 3),
                first_frame_roots=int(state["dev"][2][0]), first_frame_state_and_counts_match=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ff-iters", type=int, default=10)
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--per-scan", type=int, default=20)
    a = ap.parse_args()
    P = dict(config.LEG_FUSION, only_imu_use=True, redundancy=True)
    hip = C.CDLL(os.path.join("/opt/rocm/lib", "libamdhip64.so"))
    out = front_end(a, hip, P)
    out.update(first_frame(a, P))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
