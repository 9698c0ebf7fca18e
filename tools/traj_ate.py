#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what scoring every run of a batched run replay against ground truth costs, on the workload
of tools/runs_workload.py - R runs of K consecutive config-1 scans (only_imu_use), map = first frame + --map-scans scans, perturbed priors, replayed
once by lk_batch_replay_runs_cloud_dev so that the handle holds the bucket table.  Ground truth: the synthetic trajectory at every bucket's stamp.
One difference from the other tools' use of it: a run's scans start 0.1 s + 1 us apart, not 0.1 s.  The last point of a synthetic scan carries the
float32 offset 0.1f = 0.1 + 1.5e-9, so with back-to-back scans the last bucket of a scan is stamped 1.5 ns AFTER the first bucket of the next one, and the entry
refuses a trajectory whose stamps decrease (--scan-gap 0 shows the refusal).
  device    lk_runs_ate_dev with and without LK_ATE_ALIGN: the whole entry between two HIP events on the handle's stream (offset upload, one launch,
            the copy of the records) and as wall time, and the launch alone from the library's launch profiler;
  baseline  the only route the parent commit has: lk_runs_bucket_poses of the whole table (transfer) + association and tum.ate per run in numpy
            (compute: a vectorised nearest-stamp search and one LAPACK SVD per run), reported separately;
  replays   the plain and the recording frozen-map replay re-taken (us per scan), beside profiles/runs_cloud.json's figures.
Median over --reps timed calls after --warmup untimed ones, with min .. max.  The device's rmse is compared with the baseline's per run.
Usage: traj_ate.py [--runs R] [--scans K] [--distinct D] [--reps N] [--warmup W] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import ROOT, binding, stats
from legkilo_amd import tum  # noqa: E402

ap = rw.parser(os.path.join(ROOT, "profiles", "traj_ate.json"))
ap.add_argument("--max-dt", type=float, default=1e-3)
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

# ground truth: the true trajectory at every bucket's stamp, one packed [t x y z] table in HBM
rec0 = g.runs_bucket_poses(0, B)
gt_t = rec0["t"].copy()
gt_pos = sc.traj.pos(gt_t)
gt = np.ascontiguousarray(np.concatenate([gt_t[:, None], gt_pos], axis=1))
d_gt = g.device_malloc(gt.nbytes)
g.h2d(d_gt, gt)

timer = rw.EventTimer(g, args)
timed = timer.timed
device, last = {}, {}
for name, align in (("plain", False), ("align", True)):
    def call():
        last[name] = g.runs_ate_dev(rbo, d_gt, d_gt + 8, 32, rbo, args.max_dt, align=align)

    res = timed(call)
    kern = rw.per_launch(g, call, ("traj_ate",), args.reps, count=1)["traj_ate"]
    # bytes the launch asks for per record: the estimate's stamp twice (order check, search), the ground truth's once plus the search's last two
    # probes (the earlier ones hit the cache), and per pass over the pairs (pair + residual, with alignment also centroid + covariance) the
    # 4-byte partner word and 24 B of position from either side
    passes = 4 if align else 2
    per_rec = 8 * 2 + 8 * 3 + (4 + 48) * passes
    k = stats(kern)
    device[name] = dict(events_ms=stats([r[0] for r in res]), wall_ms=stats([r[1] for r in res]), launch_ms=k, bytes_per_record=per_rec,
                        launch_tb_per_s=per_rec * B / (k["median"] * 1e-3) / 1e12)


# ---- the parent commit's route: the table over PCIe, then numpy
def nearest(te, tg, max_dt):
    j = np.searchsorted(tg, te)
    lo, hi = np.clip(j - 1, 0, len(tg) - 1), np.clip(j, 0, len(tg) - 1)
    pick = np.where(np.abs(te - tg[lo]) <= np.abs(te - tg[hi]), lo, hi)
    keep = np.abs(te - tg[pick]) <= max_dt
    return np.flatnonzero(keep), pick[keep]


transfer, compute, host = [], {False: [], True: []}, {}
for _ in range(args.warmup + args.reps):
    t1 = time.perf_counter()
    rec = g.runs_bucket_poses(0, B)
    transfer.append((time.perf_counter() - t1) * 1e3)
    for align in (False, True):
        t1 = time.perf_counter()
        out = np.zeros(R)
        for r in range(R):
            a, b = int(rbo[r]), int(rbo[r + 1])
            i, j = nearest(rec["t"][a:b], gt_t[a:b], args.max_dt)
            out[r] = tum.ate(gt_pos[a:b][j], rec["pos"][a:b][i], align=align)
        compute[align].append((time.perf_counter() - t1) * 1e3)
        host[align] = out
baseline = dict(transfer_ms=stats(transfer[args.warmup:]), bytes=int(rec.nbytes), gb_per_s=rec.nbytes / (np.median(transfer[args.warmup:]) * 1e-3) / 1e9,
                numpy_ms=dict(plain=stats(compute[False][args.warmup:]), align=stats(compute[True][args.warmup:])))
agree = dict(plain=float(np.abs(last["plain"]["rmse"] - host[False]).max()), align=float(np.abs(last["align"]["rmse"] - host[True]).max()))
assert np.all(last["plain"]["n_pairs"] == np.diff(rbo.astype(np.int64))) and np.all(last["align"]["status"] == 0)

print(f"{R} runs x {K} config-1 scans, {B} bucket records of 144 B ({rec.nbytes / 1e6:.1f} MB), library {os.path.basename(binding.LIB_PATH)}, {args.reps} timed calls after {args.warmup}")
for name in ("plain", "align"):
    v = device[name]
    print(f"  lk_runs_ate_dev {name:5s}: {v['events_ms']['median']:.4f} ms between events ({v['events_ms']['min']:.4f} .. {v['events_ms']['max']:.4f}), wall {v['wall_ms']['median']:.4f} ms, "
          f"launch alone {v['launch_ms']['median']:.4f} ms = {v['launch_tb_per_s']:.3f} TB/s of {v['bytes_per_record']} B per record")
print(f"  baseline: lk_runs_bucket_poses {baseline['transfer_ms']['median']:.3f} ms ({baseline['gb_per_s']:.1f} GB/s) + numpy {baseline['numpy_ms']['plain']['median']:.1f} ms "
      f"(aligned {baseline['numpy_ms']['align']['median']:.1f} ms)")
print(f"  largest |rmse device - rmse numpy| over the runs: {agree['plain']:.3e} (aligned {agree['align']:.3e}); mean rmse {float(last['plain']['rmse'].mean()):.4f} m")
for name, v in replays.items():
    was = "" if stored_us is None else f" (profiles/runs_cloud.json: {stored_us[name]['median']:.3f}, {stored_us[name]['min']:.3f} .. {stored_us[name]['max']:.3f})"
    print(f"  {name:15s}: {v['median']:.3f} us per scan ({v['min']:.3f} .. {v['max']:.3f}){was}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/traj_ate.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, reps=args.reps,
                       warmup=args.warmup, max_dt=args.max_dt, scan_gap=args.scan_gap, bucket_records=B, device=device, baseline=baseline, max_abs_rmse_difference=agree,
                       replays_us_per_scan=replays, replays_us_per_scan_stored=stored_us), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_gt)
