#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: the workload of tools/overlay_runs.py - R runs of K consecutive config-1 scans with their
IMU records, replayed WITH the map insert by ONE lk_batch_replay_overlay_runs_dev call from the same map and perturbed priors - and then one slot's
overlay turned into the handle's map:
  replay     the lk_batch_replay_overlay_runs_dev call that produces the overlays;
  commit     lk_overlay_commit(slot) behind it (the base map is put back with lk_map_import before every round, untimed);
  yardstick  what a caller can do WITHOUT the commit: lk_overlay_export(slot) + lk_map_export + lk_map_import of the same map, into buffers sized
             beforehand - the transfers alone of the only route there is, without the host-side merge of the two blobs that route still needs.  It
             also runs under a library that lacks lk_overlay_commit: LEGKILO_HIP_LIB=<the parent's build> --forms replay,yardstick.
ms per call between HIP events recorded on the handle's stream around the synchronous calls (host wall time beside it): median over --reps rounds after
--warmup untimed ones, with min .. max.
Usage: overlay_commit.py [--runs R] [--scans K] [--distinct D] [--slot S] [--reps N] [--warmup W] [--forms LIST] [--commit TEXT] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # scenes.py: the synthetic room / trajectory / first-frame helpers the tests use
import lk_pkg  # noqa: E402

lk_pkg.load()
import scenes  # noqa: E402
from legkilo_amd import binding, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=1024)
ap.add_argument("--scans", type=int, default=4, help="scans per run")
ap.add_argument("--distinct", type=int, default=8, help="different trajectory segments among the runs")
ap.add_argument("--slot", type=int, default=-1, help="the slot to commit (default: the middle one)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--forms", default="replay,commit,yardstick", help="comma-separated; replay always runs (it makes the overlays)")
ap.add_argument("--map-scans", type=int, default=3, help="scans replayed live behind the first frame before the map is frozen")
ap.add_argument("--commit", default="", help="recorded in the JSON")
ap.add_argument("--json", default="")
args = ap.parse_args()
R, K, D = args.runs, args.scans, min(args.distinct, args.runs)
slot = R // 2 if args.slot < 0 else args.slot
forms = args.forms.split(",")

sc = scenes.Scene()
g = binding.LegKiloHip(sc.cfg(n_slots=R))
L = g.L
t0 = 1.0
x0 = scenes.init_filter(g, sc, t0)
scenes.first_frame(g, sc, t0, x0)
scenes.replay_vlp(g, sc, t0, args.map_scans)
base = g.map_export()
base_stats = g.map_stats()

# the D segments: K scans 0.1 s apart, each with its IMU records; run r replays segment r % D from its own perturbed prior (tools/overlay_runs.py)
seg_scans, seg_tb, seg_imu = [], [], []
for d in range(D):
    tbs = [t0 + 0.1 * (args.map_scans + 1) + 0.37 * d + 0.1 * j for j in range(K)]
    seg_scans.append([scenes.vlp_scan_input(sc, tb, 500 + K * d + j) for j, tb in enumerate(tbs)])
    seg_imu.append([synth.imu_stream(sc.traj, tb, tb + 0.1, seed=6000 + K * d + j) for j, tb in enumerate(tbs)])
    seg_tb.append(tbs)
rng = np.random.default_rng(2468)
seg_of = [r % D for r in range(R)]
scans = [s for r in range(R) for s in seg_scans[seg_of[r]]]
imus = [m for r in range(R) for m in seg_imu[seg_of[r]]]
tb = np.array([t for r in range(R) for t in seg_tb[seg_of[r]]])
run_off = (np.arange(R + 1) * K).astype(np.uint32)
scan_off = np.r_[0, np.cumsum([len(s) for s in scans])].astype(np.uint64)
n_msg = np.array([len(m) for m in imus], dtype=np.uint32)
x_run = np.array([synth.initial_state(sc.traj, t, sc.P, rng, 0.02, 0.5) for t in tb])[::K]
P_run = np.tile((1e-4 * np.eye(30)).reshape(1, 900), (R, 1))
all_pts = np.ascontiguousarray(np.concatenate(scans))
all_imu = np.ascontiguousarray(np.concatenate(imus))
d_pts, d_imu = g.device_malloc(all_pts.nbytes), g.device_malloc(all_imu.nbytes)
g.h2d(d_pts, all_pts)
g.h2d(d_imu, all_imu)

# HIP events on the handle's stream, from the runtime the library itself is linked against (already in the process)
with open("/proc/self/maps") as f:
    hip_paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln and "/torch/" not in ln})
assert hip_paths, "liblegkilo_hip.so has not brought a HIP runtime into the process"
hip = C.CDLL(hip_paths[0])
stream = C.c_void_p(g.stream())
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    assert hip.hipEventCreate(C.byref(e)) == 0


def timed(call):
    """(ms between two events around the call, ms of host wall time)"""
    assert hip.hipEventRecord(ev[0], stream) == 0
    t = time.perf_counter()
    call()
    wall = time.perf_counter() - t
    assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
    return float(ms.value), wall * 1e3


def replay():
    g.batch_replay_overlay_runs_dev(d_pts, run_off, scan_off, tb, 1, n_msg, d_imu, want_poses=False)


bufs = {}


def yardstick():
    n_ov, n_map = C.c_size_t(len(bufs["ov"])), C.c_size_t(len(bufs["map"]))
    g._chk(L.lk_overlay_export(g.h, C.c_uint32(slot), bufs["ov"].ctypes.data_as(C.c_void_p), C.byref(n_ov)))
    g._chk(L.lk_map_export(g.h, bufs["map"].ctypes.data_as(C.c_void_p), C.byref(n_map)))
    g._chk(L.lk_map_import(g.h, bufs["map"].ctypes.data_as(C.c_void_p), n_map))


t = {f: [] for f in ("replay", "commit", "yardstick")}
after_stats = None
for rep in range(args.warmup + args.reps):
    g.map_import(base)
    g.batch_set_priors(x_run, P_run)
    t["replay"].append(timed(replay))
    if "yardstick" in forms:
        need = C.c_size_t(0)   # sized untimed, in every round: an overlay's blob holds the slot's whole root table, and the pools are re-made while they warm up
        g._chk(L.lk_overlay_export(g.h, C.c_uint32(slot), None, C.byref(need)))
        if not bufs or len(bufs["ov"]) < need.value:
            bufs["ov"], bufs["map"] = np.zeros(need.value, dtype=np.uint8), np.zeros(len(base), dtype=np.uint8)
        t["yardstick"].append(timed(yardstick))
        if "commit" in forms:   # the import has changed the map as far as the library knows: the overlays again
            g.batch_set_priors(x_run, P_run)
            replay()
    if "commit" in forms:
        t["commit"].append(timed(lambda: g.overlay_commit(slot)))
        after_stats = g.map_stats()

ms = {}
for name, v in t.items():
    v = v[args.warmup:]
    if v:
        e, w = np.array([a for a, _ in v]), np.array([b for _, b in v])
        ms[name] = dict(median=float(np.median(e)), min=float(e.min()), max=float(e.max()), wall_median=float(np.median(w)))
print(f"{R} runs x {K} config-1 scans ({np.mean([len(s) for s in scans]):.0f} points per scan, {D} distinct segments), slot {slot}, {args.reps} timed rounds after "
      f"{args.warmup} warm-up rounds; base map roots / nodes / blocks {base_stats}, committed {after_stats}")
for name, label in (("replay", "lk_batch_replay_overlay_runs_dev                 "), ("commit", "lk_overlay_commit                                "),
                    ("yardstick", "lk_overlay_export + lk_map_export + lk_map_import")):
    if name in ms:
        v = ms[name]
        print(f"  {label}: {v['median']:9.3f} ms (median between events; {v['min']:.3f} .. {v['max']:.3f}; host wall {v['wall_median']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/overlay_commit.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K,
                       distinct_segments=D, slot=slot, reps=args.reps, warmup=args.warmup, points_per_scan=float(np.mean([len(s) for s in scans])),
                       base_map_roots_nodes_blocks=list(base_stats), committed_map_roots_nodes_blocks=None if after_stats is None else list(after_stats),
                       overlay_blob_bytes=len(bufs["ov"]) if bufs else None, map_blob_bytes=len(base), ms_per_call=ms), f, indent=1)
        f.write("\n")
for e in ev:
    hip.hipEventDestroy(e)
g.device_free(d_pts), g.device_free(d_imu)
g.close()
