#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what scoring every run of a batched run replay by its relative pose error costs, on the
workload of tools/runs_workload.py as tools/traj_ate.py uses it - R runs of K consecutive config-1 scans (only_imu_use), map = first frame +
--map-scans scans, perturbed priors, replayed once by lk_batch_replay_runs_cloud_dev so that the handle holds the bucket table; a run's scans start 0.1 s + 1 us apart (see traj_ate.py).
Ground truth: the synthetic trajectory's position and rotation at every bucket's stamp, one packed [t x y z r00 .. r22] table in HBM.
  device    lk_runs_rpe_dev in both delta modes (--delta seconds, --step buckets): the whole entry between two HIP events on the handle's stream
            (offset upload, one launch, the copy of the records) and as wall time, and the launch alone from the library's launch profiler;
  baseline  the only route the parent commit has: lk_runs_bucket_poses of the whole table (transfer) + tum.rpe per run in numpy (compute; timed on
            --baseline-runs runs and scaled, a run takes tens of milliseconds), reported separately;
  replays   the plain and the recording frozen-map replay re-taken (us per scan), beside profiles/runs_cloud.json's figures.
Median over --reps timed calls after --warmup untimed ones, with min .. max.  The device's figures are compared with the baseline's per run.
Usage: traj_rpe.py [--runs R] [--scans K] [--distinct D] [--reps N] [--warmup W] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import ROOT, binding, stats
from legkilo_amd import tum  # noqa: E402

ap = rw.parser(os.path.join(ROOT, "profiles", "traj_rpe.json"))
ap.add_argument("--max-dt", type=float, default=1e-3)
ap.add_argument("--delta", type=float, default=0.05, help="step in seconds")
ap.add_argument("--step", type=int, default=25, help="step in buckets (LK_RPE_INDEX)")
ap.add_argument("--baseline-runs", type=int, default=16, help="runs the numpy baseline is timed on per repetition")
ap.add_argument("--scan-gap", type=float, default=1e-6, help="seconds between the end of a scan and the start of the next one of its run")
args = ap.parse_args()

w = rw.Workload(args, scan_gap=args.scan_gap)
R, K, D, sc, g, d_pts, d_imu, x_run, P_run = w.R, w.K, w.D, w.sc, w.g, w.d_pts, w.d_imu, w.x, w.P
run_off, scan_off, tb, n_msg = w.run_off, w.scan_off, w.tb, w.n_msg


def replay(records):
    g.batch_set_priors(x_run, P_run)
    a = (d_pts, run_off, scan_off, tb, 1, n_msg, d_imu)
    t1 = time.perf_counter()
    if records:
        _, sbo = g.batch_replay_runs_cloud_dev(*a, want_poses=False, d_world=0)
    else:
        g.batch_replay_runs_dev(*a, want_poses=False)
        sbo = None
    return time.perf_counter() - t1, sbo


replays = {}
for name, records in (("plain_frozen", False), ("records_frozen", True)):   # (the recording form last: the table stays for what follows)
    replays[name] = stats([replay(records)[0] / (R * K) * 1e6 for _ in range(args.warmup + args.reps)][args.warmup:])
_, sbo = replay(True)
rbo = sbo[run_off].astype(np.uint64)
B = int(rbo[-1])
stored = os.path.join(ROOT, "profiles", "runs_cloud.json")
stored_us = {k: json.load(open(stored))["us_per_scan"][k] for k in replays} if os.path.exists(stored) else None

# ground truth: the true pose at every bucket's stamp (the runs share D segments: the rotation is evaluated once per distinct stamp)
rec0 = g.runs_bucket_poses(0, B)
gt_t = rec0["t"].copy()
uniq, inv = np.unique(gt_t, return_inverse=True)
gt_pos = sc.traj.pos(gt_t)
gt_rot = np.array([np.asarray(sc.traj.rot(float(s))).reshape(3, 3) for s in uniq])[inv]
gt = np.ascontiguousarray(np.concatenate([gt_t[:, None], gt_pos, gt_rot.reshape(-1, 9)], axis=1))
d_gt = g.device_malloc(gt.nbytes)
g.h2d(d_gt, gt)

timer = rw.EventTimer(g, args)
timed = timer.timed

MODES = (("seconds", args.delta, False), ("index", float(args.step), True))
device, last = {}, {}
for name, delta, by_index in MODES:
    def call():
        last[name] = g.runs_rpe_dev(rbo, d_gt, d_gt + 8, d_gt + 32, 104, rbo, args.max_dt, delta, by_index=by_index)

    res = timed(call)
    kern = rw.per_launch(g, call, ("traj_rpe",), args.reps, count=1)["traj_rpe"]
    device[name] = dict(delta=delta, events_ms=stats([r[0] for r in res]), wall_ms=stats([r[1] for r in res]), launch_ms=stats(kern),
                        terms=int(last[name]["n_terms"].sum()), pairs=int(last[name]["n_pairs"].sum()))

# ---- the parent commit's route: the table over PCIe, then numpy
nb = min(args.baseline_runs, R)
transfer, compute, host = [], {m[0]: [] for m in MODES}, {}
for _ in range(args.warmup + args.reps):
    t1 = time.perf_counter()
    rec = g.runs_bucket_poses(0, B)
    transfer.append((time.perf_counter() - t1) * 1e3)
    for name, delta, by_index in MODES:
        t1 = time.perf_counter()
        out = []
        for r in range(nb):
            a, b = int(rbo[r]), int(rbo[r + 1])
            out.append(tum.rpe(rec["t"][a:b], rec["pos"][a:b], rec["rot"][a:b], gt_t[a:b], gt_pos[a:b], gt_rot[a:b], args.max_dt, delta, by_index=by_index))
        compute[name].append((time.perf_counter() - t1) * 1e3 * R / nb)
        host[name] = out
baseline = dict(transfer_ms=stats(transfer[args.warmup:]), bytes=int(rec.nbytes), gb_per_s=rec.nbytes / (np.median(transfer[args.warmup:]) * 1e-3) / 1e9,
                numpy_runs_timed=nb, numpy_ms_scaled_to_all_runs={m[0]: stats(compute[m[0]][args.warmup:]) for m in MODES})
agree = {}
for name, _, _ in MODES:
    dev = last[name][:nb]
    assert all(int(dev[r]["n_terms"]) == host[name][r]["n_terms"] and int(dev[r]["n_pairs"]) == host[name][r]["n_pairs"] for r in range(nb)) and np.all(last[name]["status"] == 0)
    agree[name] = {f: float(max(abs(float(dev[r][f]) - host[name][r][f]) for r in range(nb))) for f in ("trans_rmse", "trans_max", "rot_rmse", "rot_max")}

print(f"{R} runs x {K} config-1 scans, {B} bucket records of 144 B ({rec.nbytes / 1e6:.1f} MB), library {os.path.basename(binding.LIB_PATH)}, {args.reps} timed calls after {args.warmup}")
for name, delta, _ in MODES:
    v = device[name]
    print(f"  lk_runs_rpe_dev {name:7s} (delta {delta:g}): {v['events_ms']['median']:.4f} ms between events ({v['events_ms']['min']:.4f} .. {v['events_ms']['max']:.4f}), "
          f"wall {v['wall_ms']['median']:.4f} ms, launch alone {v['launch_ms']['median']:.4f} ms; {v['terms']} terms of {v['pairs']} pairs; "
          f"mean trans_rmse {float(last[name]['trans_rmse'].mean()):.5f} m, rot_rmse {float(last[name]['rot_rmse'].mean()):.6f} rad")
print(f"  baseline: lk_runs_bucket_poses {baseline['transfer_ms']['median']:.3f} ms ({baseline['gb_per_s']:.1f} GB/s) + tum.rpe "
      + ", ".join(f"{m[0]} {baseline['numpy_ms_scaled_to_all_runs'][m[0]]['median']:.0f} ms" for m in MODES) + f" (timed on {nb} runs, scaled to {R})")
print("  largest |device - numpy| over those runs: " + "; ".join(f"{n}: " + ", ".join(f"{f} {v:.2e}" for f, v in a.items()) for n, a in agree.items()))
for name, v in replays.items():
    was = "" if stored_us is None else f" (profiles/runs_cloud.json: {stored_us[name]['median']:.3f}, {stored_us[name]['min']:.3f} .. {stored_us[name]['max']:.3f})"
    print(f"  {name:15s}: {v['median']:.3f} us per scan ({v['min']:.3f} .. {v['max']:.3f}){was}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/traj_rpe.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, reps=args.reps,
                       warmup=args.warmup, max_dt=args.max_dt, scan_gap=args.scan_gap, bucket_records=B, device=device, baseline=baseline, max_abs_difference=agree,
                       replays_us_per_scan=replays, replays_us_per_scan_stored=stored_us), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_gt)
