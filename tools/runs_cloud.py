#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what the per-bucket poses and the registered cloud of the run replays cost, on the workload
of tools/runs_workload.py - R runs of K consecutive config-1 scans (only_imu_use: each scan with its IMU records), map = first frame + --map-scans
scans, perturbed priors.  Forms, per entry (frozen: lk_batch_replay_runs_dev, overlay: lk_batch_replay_overlay_runs_dev):
  plain_*    the EXISTING entry.  These two also run under a library that lacks the new entries (LEGKILO_HIP_LIB=<the parent's build> --forms
             plain_frozen,plain_overlay --json PARENT.json); a later run with --parent-json PARENT.json records both and says whether the new median lies
             inside the parent's min .. max range widened by the new run's own range - run-to-run spread is the only margin there is;
  records_*  the _cloud entry with scan_bucket_off only: the bucket table recorded, no cloud;
  cloud_*    the _cloud entry with the table and d_world_out;
  register   lk_register_cloud_kernel alone, between HIP events (the library's launch profiler, lk_profile_enable): 32 bytes moved per point;
  live       the route this replaces: lk_run_scans_dev with d_world_out, run after run on slot 0 (map, state and times put back before every run), over
             the first --live-runs runs.
us per scan: median over --reps timed calls after --warmup untimed ones, with min .. max; the priors are armed outside the timed region.
Usage: runs_cloud.py [--runs R] [--scans K] [--distinct D] [--reps N] [--warmup W] [--live-runs L] [--forms LIST] [--parent-json PATH] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding

ALL = "plain_frozen,records_frozen,cloud_frozen,plain_overlay,records_overlay,cloud_overlay,register,live"
COPY_CEILING_TBS = 6.29   # the measured device-to-device copy rate of this card

ap = rw.parser()
ap.add_argument("--forms", default=ALL, help="comma-separated, measured in this order")
ap.add_argument("--live-runs", type=int, default=16, help="runs of the live form (it costs ~6 ms per scan)")
ap.add_argument("--parent-json", default="", help="this tool's JSON of the plain forms under the parent commit's library, same machine, same session")
args = ap.parse_args()
forms = args.forms.split(",")

w = rw.Workload(args)
R, K, D, g, d_pts, d_imu, n_pts, x_run, P_run = w.R, w.K, w.D, w.g, w.d_pts, w.d_imu, w.n_pts, w.x, w.P
run_off, scan_off, tb, n_msg, msg_off = w.run_off, w.scan_off, w.tb, w.n_msg, w.msg_off
start = (g.map_export(), g.get_last_slide_position())
d_world = g.device_malloc(16 * n_pts)
n_buckets = 0


def replay(overlay, cloud, records):
    global n_buckets
    g.batch_set_priors(x_run, P_run)
    a = (d_pts, run_off, scan_off, tb, 1, n_msg, d_imu)
    t1 = time.perf_counter()
    if not (cloud or records):
        (g.batch_replay_overlay_runs_dev if overlay else g.batch_replay_runs_dev)(*a, want_poses=False)
    else:
        _, sbo = (g.batch_replay_overlay_runs_cloud_dev if overlay else g.batch_replay_runs_cloud_dev)(*a, want_poses=False, d_world=d_world if cloud else 0)
        n_buckets = int(sbo[-1])
    return time.perf_counter() - t1


def register_form():
    """The registration launch of one frozen-map _cloud call, timed by the library between two HIP events."""
    g.batch_set_priors(x_run, P_run)
    g.profile_reset()
    g.profile_enable(True)
    try:
        g.batch_replay_runs_cloud_dev(d_pts, run_off, scan_off, tb, 1, n_msg, d_imu, want_poses=False, d_world=d_world)
    finally:
        g.profile_enable(False)
    n, ms = g.profile_get("register_cloud")
    assert n == 1, n
    return ms * 1e-3


L = min(args.live_runs, R)


def live_form():
    total = 0.0
    for r in range(L):
        g.map_import(start[0])
        g.set_last_slide_position(start[1])
        g.set_state(x_run[r], P_run[0].reshape(30, 30))
        g.set_times(tb[r * K], tb[r * K])
        s0 = r * K
        t1 = time.perf_counter()
        g.run_scans_dev(d_pts, scan_off[s0:s0 + K + 1], tb[s0:s0 + K], 1, n_msg[s0:s0 + K], d_imu + 56 * int(msg_off[s0]), d_world=d_world)
        total += time.perf_counter() - t1
    return total


known = dict(plain_frozen=(lambda: replay(False, False, False), R * K), records_frozen=(lambda: replay(False, False, True), R * K),
             cloud_frozen=(lambda: replay(False, True, True), R * K), plain_overlay=(lambda: replay(True, False, False), R * K),
             records_overlay=(lambda: replay(True, False, True), R * K), cloud_overlay=(lambda: replay(True, True, True), R * K),
             register=(register_form, R * K), live=(live_form, L * K))
us = {}
for name in forms:
    form, n = known[name]
    v = [form() / n * 1e6 for _ in range(args.warmup + args.reps)][args.warmup:]
    us[name] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), scans=n)
    if name == "live":
        g.map_import(start[0])   # (the live form changed the handle's map)
        us[name]["runs"] = f"the first {L} of the {R} runs, one after another"
if "register" in us:
    v = us["register"]
    sec = v["median"] * 1e-6 * R * K
    v.update(points=n_pts, buckets=n_buckets, bytes_moved=32 * n_pts, ms_per_call=sec * 1e3, tb_per_s=32 * n_pts / sec / 1e12,
             share_of_copy_ceiling=32 * n_pts / sec / 1e12 / COPY_CEILING_TBS, copy_ceiling_tb_per_s=COPY_CEILING_TBS)

parent, verdict = None, {}
if args.parent_json:
    parent = json.load(open(args.parent_json))
    for name in ("plain_frozen", "plain_overlay"):
        if name in us and name in parent["us_per_scan"]:
            p, n = parent["us_per_scan"][name], us[name]
            spread = n["max"] - n["min"]
            verdict[name] = dict(parent_range=[p["min"], p["max"]], new_median=n["median"], new_spread=spread,
                                 inside=bool(p["min"] - spread <= n["median"] <= p["max"] + spread))

pps = n_pts / (R * K)
print(f"{R} runs x {K} config-1 scans ({pps:.0f} points per scan, {D} distinct segments), library {os.path.basename(binding.LIB_PATH)}, {args.reps} timed calls after {args.warmup} warm-up calls")
for name in forms:
    v = us[name]
    print(f"  {name:16s}: {v['median']:9.3f} us per scan (median; {v['min']:.3f} .. {v['max']:.3f})")
if "register" in us:
    v = us["register"]
    print(f"  registration alone: {v['ms_per_call']:.4f} ms for {n_pts} points in {n_buckets} buckets = {v['tb_per_s']:.3f} TB/s, {100 * v['share_of_copy_ceiling']:.1f} % of the {COPY_CEILING_TBS} TB/s copy ceiling")
for name, v in verdict.items():
    print(f"  {name}: parent {v['parent_range'][0]:.3f} .. {v['parent_range'][1]:.3f}, new median {v['new_median']:.3f} (own spread {v['new_spread']:.3f}): {'inside' if v['inside'] else 'OUTSIDE'}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/runs_cloud.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D,
                       reps=args.reps, warmup=args.warmup, map_scans=args.map_scans, points_per_scan=pps, us_per_scan=us,
                       parent=None if parent is None else dict(library=parent["library"], us_per_scan=parent["us_per_scan"]), plain_entries_vs_parent=verdict), f, indent=1)
        f.write("\n")
w.close(d_world)
