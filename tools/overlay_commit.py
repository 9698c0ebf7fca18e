#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: the workload of tools/runs_workload.py - R runs of K consecutive config-1 scans with their
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
import ctypes as C
import json
import os

import numpy as np

import runs_workload as rw
from runs_workload import binding

ap = rw.parser()
ap.add_argument("--slot", type=int, default=-1, help="the slot to commit (default: the middle one)")
ap.add_argument("--forms", default="replay,commit,yardstick", help="comma-separated; replay always runs (it makes the overlays)")
args = ap.parse_args()
forms = args.forms.split(",")

w = rw.Workload(args, per_scan=True)   # (the draws of tools/overlay_runs.py: a prior per scan, a run starts from its first scan's)
R, K, D, g, d_pts, d_imu, run_off, scan_off, tb, n_msg = w.R, w.K, w.D, w.g, w.d_pts, w.d_imu, w.run_off, w.scan_off, w.tb, w.n_msg
slot = R // 2 if args.slot < 0 else args.slot
L = g.L
base = g.map_export()
base_stats = g.map_stats()
x_run, P_run = w.x[::K], w.P
pps = w.n_pts / (R * K)
timer = rw.EventTimer(g, args)
timed = timer.once


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
        e, wall = np.array([a for a, _ in v]), np.array([b for _, b in v])
        ms[name] = dict(median=float(np.median(e)), min=float(e.min()), max=float(e.max()), wall_median=float(np.median(wall)))
print(f"{R} runs x {K} config-1 scans ({pps:.0f} points per scan, {D} distinct segments), slot {slot}, {args.reps} timed rounds after "
      f"{args.warmup} warm-up rounds; base map roots / nodes / blocks {base_stats}, committed {after_stats}")
for name, label in (("replay", "lk_batch_replay_overlay_runs_dev                 "), ("commit", "lk_overlay_commit                                "),
                    ("yardstick", "lk_overlay_export + lk_map_export + lk_map_import")):
    if name in ms:
        v = ms[name]
        print(f"  {label}: {v['median']:9.3f} ms (median between events; {v['min']:.3f} .. {v['max']:.3f}; host wall {v['wall_median']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/overlay_commit.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K,
                       distinct_segments=D, slot=slot, reps=args.reps, warmup=args.warmup, points_per_scan=pps,
                       base_map_roots_nodes_blocks=list(base_stats), committed_map_roots_nodes_blocks=None if after_stats is None else list(after_stats),
                       overlay_blob_bytes=len(bufs["ov"]) if bufs else None, map_blob_bytes=len(base), ms_per_call=ms), f, indent=1)
        f.write("\n")
timer.close()
w.close()
