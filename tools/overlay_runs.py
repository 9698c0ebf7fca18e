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
import argparse
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--forms", default="independent,runs,live", help="comma-separated, measured in this order")
ap.add_argument("--live-runs", type=int, default=16, help="runs of the live form (it costs ~4 ms per scan)")
ap.add_argument("--map-scans", type=int, default=3, help="scans replayed live behind the first frame before the map is frozen")
ap.add_argument("--commit", default="", help="recorded in the JSON")
ap.add_argument("--json", default="")
args = ap.parse_args()
R, K, D = args.runs, args.scans, min(args.distinct, args.runs)

sc = scenes.Scene()
g = binding.LegKiloHip(sc.cfg(n_slots=R))
t0 = 1.0
x0 = scenes.init_filter(g, sc, t0)
scenes.first_frame(g, sc, t0, x0)
scenes.replay_vlp(g, sc, t0, args.map_scans)
start = (g.map_export(), g.get_last_slide_position())

# the D segments: K scans 0.1 s apart, each with its IMU records; run r replays segment r % D from its own perturbed prior
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
msg_off = np.r_[0, np.cumsum(n_msg)]
x_scan = np.array([synth.initial_state(sc.traj, t, sc.P, rng, 0.02, 0.5) for t in tb])   # a prior per scan: the independent form's; a run starts from its first scan's
P_scan = np.tile((1e-4 * np.eye(30)).reshape(1, 900), (R, 1))
all_pts = np.ascontiguousarray(np.concatenate(scans))
all_imu = np.ascontiguousarray(np.concatenate(imus))
d_pts, d_imu = g.device_malloc(all_pts.nbytes), g.device_malloc(all_imu.nbytes)
g.h2d(d_pts, all_pts)
g.h2d(d_imu, all_imu)
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
print(f"{R} runs x {K} config-1 scans ({np.mean([len(s) for s in scans]):.0f} points per scan, {D} distinct segments), {args.reps} timed calls after {args.warmup} warm-up calls")
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
                       points_per_scan=float(np.mean([len(s) for s in scans])), ms_per_scan=ms, runs_over_independent=ratio), f, indent=1)
        f.write("\n")
g.device_free(d_pts), g.device_free(d_imu)
g.close()
