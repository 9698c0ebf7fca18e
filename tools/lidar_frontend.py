"""Time of the lidar front end of a recorded run on the device: lk_decode_scans_dev (one call for the whole run) next to the per-scan loop
lk_decode_scan_dev + lk_preprocess_scan_dev over the SAME device-resident bytes, on two workloads:

    vlp16   1 024 VLP-16-shaped messages (Velodyne layout, 22 B per point, up to 28 800 points each), filter_num 3, blind 1.5, leaf 0.3
    ouster  256 config-4 messages (bench.py's OUSTER_MSG_LAYOUT, 16 B per point, up to 65 536 points each), diter.yaml's filter_num / blind /
            time_scale, leaf 0.5

Each workload tiles --distinct generated scans with increasing header stamps (one VLP-16 scan takes ~66 ms to generate), packs them at odd
byte offsets with gaps, and uploads them once.  The batch call is timed between HIP events on the handle's stream in steady state after
warm-up (median and minimum); the loop likewise, around all its calls (it includes the host round trips of every call and the ctypes
overhead of this Python driver).  outputs_bit_equal: the loop's scans, written back to back, equal the batch call's byte for byte, and so
do the begin / end times.  The ouster workload also times ONE message through both paths.

    python tools/lidar_frontend.py [--iters 20] [--warmup 3] [--loop-iters 3] [--batch-only]

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import lk_pkg  # noqa: E402

lk_pkg.load()
from legkilo_amd import binding, config, synth  # noqa: E402

OUSTER_MSG_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<u4")])   # bench.py's config-4 message
OUSTER_MSG_LAYOUT = dict(point_step=16, off_x=0, off_y=4, off_z=8, off_time=12, lidar_type=2)


def vlp16_workload(n_msgs, distinct, t0=2.0):
    P = config.LEG_FUSION
    world, traj = synth.World(), synth.Trajectory()
    base = [synth.vlp16_scan(world, traj, t0 + 0.1 * k, P, seed_noise=3003 + k) for k in range(distinct)]
    msgs = [synth.cloud_message(base[k % distinct], 1, t0 + 0.1 * k, seed=k % distinct) for k in range(n_msgs)]
    return msgs, t0 + 0.1 * np.arange(n_msgs), synth.cloud_layout(1), 1.0, P["filter_num"], P["blind"], 0.3, P


def ouster_workload(n_msgs, distinct, t0=3.0):
    P = config.DITER
    world, traj = synth.World(), synth.Trajectory()
    base = []
    for k in range(distinct):
        pts, t_ns = synth.ouster_scan(world, traj, t0 + 0.1 * k, P, seed_noise=4000 + k)
        raw = np.zeros(len(pts), dtype=OUSTER_MSG_DTYPE)
        raw["x"], raw["y"], raw["z"], raw["t"] = pts["x"], pts["y"], pts["z"], t_ns
        base.append(raw)
    msgs = [base[k % distinct] for k in range(n_msgs)]
    return msgs, t0 + 0.1 * np.arange(n_msgs), OUSTER_MSG_LAYOUT, P["time_scale"], P["filter_num"], P["blind"], P["voxel_grid_resolution"], P


class Timer:
    def __init__(self, stream):
        self.hip = C.CDLL(os.path.join("/opt/rocm/lib", "libamdhip64.so"))
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0
        self.stream = C.c_void_p(stream)

    def __call__(self, fn):
        self.hip.hipEventRecord(self.ev[0], self.stream)
        r = fn()
        self.hip.hipEventRecord(self.ev[1], self.stream)
        self.hip.hipEventSynchronize(self.ev[1])
        ms = C.c_float()
        self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1])
        return ms.value, r

    def close(self):
        for e in self.ev:
            self.hip.hipEventDestroy(e)


def measure(name, work, a):
    g0 = time.perf_counter()
    msgs, stamps, layout, scale, fn, blind, leaf, P = work
    buf, msg_off, n_points = synth.pack_cloud_run(msgs, seed=1)
    gen_s = time.perf_counter() - g0
    S, total, n_max = len(msgs), int(n_points.sum()), int(n_points.max())
    g = binding.LegKiloHip(config.make_config(P, max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12))
    tm = Timer(g.stream())
    d_msgs, d_out, d_loop = g.device_malloc(buf.nbytes), g.device_malloc(total * 16), g.device_malloc(total * 16)
    d_dec, d_ds = g.device_malloc(n_max * 16), g.device_malloc(n_max * 16)
    g.h2d(d_msgs, buf)

    def batch(m=S):
        return g.decode_scans_dev(d_msgs, msg_off[:m], n_points[:m], stamps[:m], layout, scale, fn, blind, leaf, d_out)

    def loop(m=S):
        off, tb, te = 0, np.zeros(m), np.zeros(m)
        for s in range(m):
            n, tb[s], te[s] = g.decode_scan_dev(d_msgs + int(msg_off[s]), int(n_points[s]), layout, scale, fn, blind, float(stamps[s]), d_dec)
            off += g.preprocess_scan_dev(d_dec, n, leaf, d_loop + 16 * off)
        return off, tb, te

    b_ms, l_ms = [], []
    for it in range(a.warmup + a.iters):
        ms, (so, tb, te) = tm(batch)
        if it >= a.warmup:
            b_ms.append(ms)
    if a.batch_only:
        for d in (d_msgs, d_out, d_loop, d_dec, d_ds):
            g.device_free(d)
        tm.close()
        g.close()
        return dict(messages=S, raw_points=total, points_out=int(so[-1]), batch_ms_median=round(float(np.median(b_ms)), 3))
    for it in range(1 + a.loop_iters):
        ms, (n_loop, ltb, lte) = tm(loop)
        if it >= 1:
            l_ms.append(ms)
    out_b = np.zeros(int(so[-1]) * 16, dtype=np.uint8)
    out_l = np.zeros(n_loop * 16, dtype=np.uint8)
    g.d2h(out_b, d_out)
    g.d2h(out_l, d_loop)
    same = bool(n_loop == int(so[-1]) and np.array_equal(out_b, out_l) and np.array_equal(tb, ltb) and np.array_equal(te, lte))
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    r = dict(messages=S, raw_points=total, bytes=int(buf.nbytes), points_out=int(so[-1]), point_step=layout["point_step"],
             batch_ms_median=med(b_ms), batch_ms_min=round(min(b_ms), 3), per_scan_loop_ms_median=med(l_ms), per_scan_loop_ms_min=round(min(l_ms), 3),
             speedup_median=round(float(np.median(l_ms) / np.median(b_ms)), 1), outputs_bit_equal=same, pack_s=round(gen_s, 1))
    if name == "ouster":   # one message through both paths (what the per-scan entries would pay as the one-message case of the batch body)
        one_b = [tm(lambda: batch(1))[0] for _ in range(a.warmup + a.iters)][a.warmup:]
        one_l = [tm(lambda: loop(1))[0] for _ in range(a.warmup + a.iters)][a.warmup:]
        r.update(one_message_batch_ms_median=med(one_b), one_message_per_scan_ms_median=med(one_l))
    for d in (d_msgs, d_out, d_loop, d_dec, d_ds):
        g.device_free(d)
    tm.close()
    g.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-iters", type=int, default=3, help="timed repetitions of the per-scan loop (after one warm-up pass)")
    ap.add_argument("--vlp16-messages", type=int, default=1024)
    ap.add_argument("--ouster-messages", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=64, help="generated scans per workload, tiled to the message count")
    ap.add_argument("--batch-only", action="store_true", help="time the batch call only (no loop, no comparison): for a kernel trace of the batch call")
    a = ap.parse_args()
    res = dict(iters=a.iters, warmup=a.warmup, loop_iters=a.loop_iters, distinct_scans=a.distinct)
    res["vlp16"] = measure("vlp16", vlp16_workload(a.vlp16_messages, a.distinct), a)
    res["ouster"] = measure("ouster", ouster_workload(a.ouster_messages, a.distinct), a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
