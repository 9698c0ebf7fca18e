#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: R runs of K consecutive config-1 scans (only_imu_use: each scan with its IMU records)
replayed on the FROZEN map - first frame + --map-scans scans, the workload of tools/runs_workload.py - from the same perturbed priors in three forms:
  runs        ONE lk_batch_replay_runs_dev call: a run per filter slot, state, covariance and time stamps carried from scan to scan;
  chunks      the same runs as two calls, the first K / 2 scans of every run and then the rest with LK_RUNS_CONTINUE;
  independent the same R*K scans, cut to n_slots = R at a time, as independent scans through lk_batch_replay_scans_imu_dev (K calls, every scan
              from a prior of its own): the yardstick - per bucket the run kernel does the scan kernel's work plus one comparison, and 15 stores
              per scan.  This form alone also runs under a library that lacks the new entry (LEGKILO_HIP_LIB=<the parent's build> --forms independent).
us per scan: median over --reps timed calls after --warmup untimed ones, with min .. max; the priors are armed outside the timed region.
Usage: replay_runs.py [--runs R] [--scans K] [--distinct D] [--reps N] [--warmup W] [--forms LIST] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding

ap = rw.parser()
ap.add_argument("--forms", default="independent,runs,chunks", help="comma-separated, measured in this order")
args = ap.parse_args()

w = rw.Workload(args, per_scan=True)   # a prior per scan: the independent form's; a run starts from its first scan's
R, K, D, g, seg_scans, tables, whole, d_pts, d_imu = w.R, w.K, w.D, w.g, w.seg_scans, w.tables, w.t, w.d_pts, w.d_imu
tb_flat, x_scan, P_scan = w.tb, w.x, w.P
# the two chunks of a run are not contiguous in the run-major arrays: each half gets arrays of its own
half = K // 2
parts = []
if "chunks" in args.forms.split(","):
    assert 1 <= half < K
    for lo, hi in ((0, half), (half, K)):
        t = tables(lo, hi)
        t["d_pts"], t["d_imu"] = w.upload(t)
        parts.append(t)
# the independent form: R consecutive scans of the run-major array at a time (runs of K: call c holds the runs c R / K .. (c + 1) R / K whole)
indep = []
for c in range(K):
    lo, hi = c * R, (c + 1) * R
    indep.append((d_pts + 16 * int(whole["scan_off"][lo]), whole["scan_off"][lo:hi + 1] - whole["scan_off"][lo], tb_flat[lo:hi], whole["n_msg"][lo:hi],
                  d_imu + 56 * int(whole["msg_off"][lo]), x_scan[lo:hi]))


def runs_form():
    g.batch_set_priors(x_scan[::K], P_scan)
    t = time.perf_counter()
    g.batch_replay_runs_dev(d_pts, whole["run_off"], whole["scan_off"], tb_flat, 1, whole["n_msg"], d_imu, want_poses=False)
    return time.perf_counter() - t


def chunks_form():
    g.batch_set_priors(x_scan[::K], P_scan)
    t = time.perf_counter()
    for i, p in enumerate(parts):
        g.batch_replay_runs_dev(p["d_pts"], p["run_off"], p["scan_off"], p["t_begin"], 1, p["n_msg"], p["d_imu"], cont=i > 0, want_poses=False)
    return time.perf_counter() - t


def independent_form():
    total = 0.0
    for dp, so, tb, nm, dm, xs in indep:
        g.batch_set_priors(xs, P_scan)
        t = time.perf_counter()
        g.batch_replay_scans_imu_dev(dp, so, tb, nm, dm, want_poses=False)
        total += time.perf_counter() - t
    return total


us = {}
known = dict(runs=runs_form, chunks=chunks_form, independent=independent_form)
for name in args.forms.split(","):
    t = [known[name]() / (R * K) * 1e6 for _ in range(args.warmup + args.reps)][args.warmup:]
    us[name] = dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), scans=R * K)
ratio = us["runs"]["median"] / us["independent"]["median"] if "runs" in us and "independent" in us else None
pps = float(np.mean([len(s) for seg in seg_scans for s in seg]))
print(f"{R} runs x {K} config-1 scans ({pps:.0f} points per scan, {D} distinct segments), frozen map, {args.reps} timed calls after {args.warmup} warm-up calls")
for name, label in (("runs", "one lk_batch_replay_runs_dev            "), ("chunks", f"two continued calls, {half} + {K - half} scans      "),
                    ("independent", f"{K} x lk_batch_replay_scans_imu_dev       ")):
    if name in us:
        v = us[name]
        print(f"  {label}: {v['median']:9.2f} us per scan (median; {v['min']:.2f} .. {v['max']:.2f})")
if ratio is not None:
    print(f"  runs / independent: {ratio:.3f}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/replay_runs.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D,
                       reps=args.reps, warmup=args.warmup, map_scans=args.map_scans, points_per_scan=pps, us_per_scan=us, runs_over_independent=ratio), f, indent=1)
        f.write("\n")
for t in parts:
    g.device_free(t["d_pts"]), g.device_free(t["d_imu"])
w.close()
