#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: R runs of K consecutive config-1 scans (only_imu_use: each scan with its IMU records),
replayed WITH the map insert in three ways from the same map and the same perturbed priors -
  runs       ONE lk_batch_replay_overlay_runs_dev call: a run per filter slot, state, covariance, times and overlay carried from scan to scan;
  independent the same R*K scans, cut to n_slots = R at a time, as independent scans through lk_batch_replay_overlay_ragged_dev (K calls; every scan from
             a prior of its own, its overlay empty): the yardstick - a run pays the same bucket chains, plus overlays that grow;
  live       lk_run_scans_dev run after run on slot 0 (map, state and times put back before every run), over the first --live-runs runs.
ms per scan: median over --reps timed calls after --warmup untimed ones, with min .. max.  (Two warm-up calls by default: in the first the overlay
pools grow from their first guess, in the second they are re-made once from the first one's high-water marks; from the third on they stay.)
--forms picks the forms (the independent one alone also runs under a library that lacks the new entry: LEGKILO_HIP_LIB=<the parent's build>).
The runs are --distinct different segments of the trajectory, repeated over the R slots under different priors (Monte-Carlo starts of a segment).
Usage: overlay_runs.py [--runs R] [--scans K] [--distinct D] [--reps N] [--warmup W] [--live-runs L] [--forms LIST] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding, synth

ap = rw.parser()
ap.add_argument("--forms", default="independent,runs,live", help="comma-separated, measured in this order")
ap.add_argument("--live-runs", type=int, default=16, help="runs of the live form (it costs ~4 ms per scan)")
args = ap.parse_args()

w = rw.Workload(args, per_scan=True)   # (tools/runs_workload.py) a prior per scan: the independent form's; a run starts from its first scan's
R, K, D, g, seg_scans, seg_of, d_pts, d_imu = w.R, w.K, w.D, w.g, w.seg_scans, w.seg_of, w.d_pts, w.d_imu
run_off, scan_off, tb, n_msg, msg_off, x_scan, P_scan = w.run_off, w.scan_off, w.tb, w.n_msg, w.msg_off, w.x, w.P
start = (g.map_export(), g.get_last_slide_position())
imus = [m for r in range(R) for m in w.seg_imu[seg_of[r]]]
pps = w.n_pts / (R * K)
tabs = [synth.buckets_of(s) for seg in seg_scans for s in seg]   # host tables of the independent form, per distinct scan
tab_of = [seg_of[r] * K + j for r in range(R) for j in range(K)]
chunks = []
for c in range(K):   # the flat scan array cut to R at a time
    lo, hi = c * R, (c + 1) * R
    chunks.append((int(scan_off[lo]), g.ragged_tables(scan_off[lo:hi + 1] - scan_off[lo], [tabs[tab_of[s]][0] for s in range(lo, hi)],
                                                      [tabs[tab_of[s]][1] for s in range(lo, hi)], tb[lo:hi], imus=imus[lo:hi]), x_scan[lo:hi]))


def runs_form():
    g.batch_set_priors(x_scan[::K], P_scan)
    t = time.perf_counter()
    g.batch_replay_overlay_runs_dev(d_pts, run_off, scan_off, tb, 1, n_msg, d_imu, want_poses=False)
    return time.perf_counter() - t


def independent_form():
    total = 0.0
    for first, tables, xs in chunks:
        g.batch_set_priors(xs, P_scan)
        t = time.perf_counter()
        g.batch_replay_overlay_ragged_dev(d_pts + 16 * first, tables, want_poses=False)
        total += time.perf_counter() - t
    return total


L = min(args.live_runs, R)


def live_form():
    total = 0.0
    for r in range(L):
        g.map_import(start[0])
        g.set_last_slide_position(start[1])
        g.set_state(x_scan[r * K], P_scan[0].reshape(30, 30))
        g.set_times(tb[r * K], tb[r * K])
        s0 = r * K
        t = time.perf_counter()
        g.run_scans_dev(d_pts, scan_off[s0:s0 + K + 1], tb[s0:s0 + K], 1, n_msg[s0:s0 + K], d_imu + 56 * int(msg_off[s0]))
        total += time.perf_counter() - t
    return total


ms = {}
known = dict(runs=(runs_form, R * K), independent=(independent_form, R * K), live=(live_form, L * K))
for name in args.forms.split(","):
    form, n = known[name]
    t = [form() / n * 1e3 for _ in range(args.warmup + args.reps)][args.warmup:]
    ms[name] = dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), scans=n)
    if name == "runs":
        ms[name]["resident_rounds"] = g.overlay_resident_rounds()
        ms[name]["pool_bytes"], ms[name]["root_entries"] = g.overlay_pool_bytes()[:2]
        ms[name]["high_water_roots_nodes_blocks"] = list(g.overlay_stats())
    if name == "independent":
        ms[name]["resident_rounds"] = g.overlay_resident_rounds()
        ms[name]["pool_bytes"], ms[name]["root_entries"] = g.overlay_pool_bytes()[:2]
g.map_import(start[0])   # (the live form changed the handle's map)
ratio = ms["runs"]["median"] / ms["independent"]["median"] if "runs" in ms and "independent" in ms else None
print(f"{R} runs x {K} config-1 scans ({pps:.0f} points per scan, {D} distinct segments), {args.reps} timed calls after {args.warmup} warm-up calls")
for name, label in (("runs", "one lk_batch_replay_overlay_runs_dev      "), ("independent", f"{K} x lk_batch_replay_overlay_ragged_dev    "),
                    ("live", f"lk_run_scans_dev, {L} runs one after another")):
    if name in ms:
        v = ms[name]
        print(f"  {label}: {v['median'] * 1e3:9.2f} us per scan (median; {v['min'] * 1e3:.2f} .. {v['max'] * 1e3:.2f})")
if ratio is not None:
    print(f"  runs / independent: {ratio:.3f}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/overlay_runs.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D,
                       reps=args.reps, warmup=args.warmup,
                       points_per_scan=pps, ms_per_scan=ms, runs_over_independent=ratio), f, indent=1)
        f.write("\n")
w.close()
