"""Time of the leg kinematics front end on the device: lk_decode_highstate_dev + lk_kin_split_dev on a recorded-run-sized input - 1 024 scans x
50 HighState messages (51 200 x 1 095 B = 56 MB in HBM), every message kept (the IMU changes on every message) - in steady state after warm-up,
between HIP events on the handle's stream, next to the numpy restatement's CPU time (tests/kin_ref.py) for the same work.

    python tools/highstate_frontend.py [--iters 50] [--warmup 5]

Prints one JSON line.  Both entries are synchronous (each reads back a few words), so the event interval includes their host round trips."""
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
import kin_ref  # noqa: E402
from legkilo_amd import abi, binding, config, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--per-scan", type=int, default=50)
    a = ap.parse_args()
    P = dict(config.DITER, redundancy=True)
    n = a.scans * a.per_scan
    t0 = 2.0
    msgs, _ = synth.highstate_stream(synth.Trajectory(), t0, t0 + n / 500.0, P, hold=1, seed=123)
    assert len(msgs) == n
    ends = t0 + (np.arange(a.scans) + 1) * (a.per_scan / 500.0) - 1.5e-3   # between two messages; the newest message lies beyond the last end

    hip = C.CDLL(os.path.join("/opt/rocm/lib", "libamdhip64.so"))
    g = binding.LegKiloHip(config.make_config(P, max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12))
    d_msgs = g.device_malloc(msgs.nbytes)
    d_kins = g.device_malloc(n * synth.KIN_DTYPE.itemsize)
    g.h2d(d_msgs, msgs)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    stream = C.c_void_p(g.stream())
    dec_ms, split_ms, wall_ms = [], [], []
    for it in range(a.warmup + a.iters):
        g.kin_configure(P)   # host-side reset: every iteration decodes the same stream from the start
        w0 = time.perf_counter()
        hip.hipEventRecord(ev[0], stream)
        k = g.decode_highstate_dev(d_msgs, n, d_kins)
        hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        d_ms = ms.value
        hip.hipEventRecord(ev[0], stream)
        n_msg, npk, ncs = g.kin_split_dev(d_kins, k, ends)
        hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        w1 = time.perf_counter()
        if it >= a.warmup:
            dec_ms.append(d_ms)
            split_ms.append(ms.value)
            wall_ms.append((w1 - w0) * 1e3)
    assert k == n and npk == a.scans and ncs == n - 1, (k, npk, ncs)
    # the numpy restatement of the same work (one run: it takes seconds)
    c0 = time.perf_counter()
    ref = kin_ref.Frontend(P).process(msgs)
    kin_ref.sync_package(ref["time_stamp"], ends)
    cpu_ms = (time.perf_counter() - c0) * 1e3
    recs = np.zeros(k, dtype=synth.KIN_DTYPE)
    g.d2h(recs, d_kins)
    same = bool(np.array_equal(recs["time_stamp"], ref["time_stamp"]) and np.array_equal(recs["contact"], ref["contact"]))
    g.device_free(d_msgs)
    g.device_free(d_kins)
    g.close()
    for e in ev:
        hip.hipEventDestroy(e)
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps(dict(messages=n, scans=a.scans, bytes=int(msgs.nbytes), kept=int(k), iters=a.iters,
                          decode_ms_median=round(med(dec_ms), 4), decode_ms_min=round(min(dec_ms), 4),
                          split_ms_median=round(med(split_ms), 4), split_ms_min=round(min(split_ms), 4),
                          wall_ms_median=round(med(wall_ms), 4), numpy_restatement_ms=round(cpu_ms, 1), records_match_restatement=same,
                          highstate_bytes=abi.LK_HIGHSTATE_BYTES)))


if __name__ == "__main__":
    main()
