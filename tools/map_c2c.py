#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what scoring map clouds against a reference cloud costs (lk_clouds_c2c_dev), on the
workload of tools/runs_workload.py as tools/map_clouds.py uses it - R runs of K consecutive config-1 scans replayed on the frozen map with
d_world_out, cut into one file per run and downsampled (lk_downsample_clouds_dev); its d_out / out_off are the map clouds and stay in HBM.  The reference cloud ("survey") is the union of the
first --ref-files map clouds downsampled once more as one file.  Forms, at every max_dist of --max-dist:
  accuracy      pairs (f, 0): every map cloud as query against the survey;
  completeness  pairs (0, f): the survey as query against every map cloud (the sides exchanged: R search structures, one segment each).
ms per call: median over --reps timed calls after --warmup untimed ones, with min .. max, between two HIP events on the handle's stream (the call is
synchronous, the events bracket it) and by the host's wall clock; then, in profiling mode (every launch between its own events), the grid build
(bounds, grid, keys, gather - the sort is not a launch of the library's and is the remainder) and the query and reduce launches on their own.
Baseline, the only route the parent commit has: lk_memcpy_d2h of the map clouds and the survey, then scipy.spatial.cKDTree on the host when scipy
imports (a tree per reference cloud, wall clock, over the first --host-files files, scaled by query points), else legkilo_amd.cloudmetrics.c2c the
same way; the matched counts of those files are compared with the device's and the largest difference is recorded.
The run replay and lk_downsample_clouds_dev are timed before and after the C2C calls (tools/runs_cloud.py's and tools/map_clouds.py's figures).
Usage: map_c2c.py [--runs R] [--scans K] [--distinct D] [--leaf M] [--max-dist LIST] [--ref-files F] [--reps N] [--warmup W] [--host-files F] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding, both, stats
from legkilo_amd import cloudmetrics  # noqa: E402

try:
    from scipy.spatial import cKDTree
except ImportError:
    cKDTree = None

ap = rw.parser()
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--max-dist", default="0.25,0.05")
ap.add_argument("--ref-files", type=int, default=8, help="map clouds whose union, downsampled once more, is the reference cloud")
ap.add_argument("--host-files", type=int, default=16, help="files of the host baseline")
args = ap.parse_args()

w = rw.Workload(args)
R, K, D, g, d_pts, d_imu, n_pts, x_run, P_run = w.R, w.K, w.D, w.g, w.d_pts, w.d_imu, w.n_pts, w.x, w.P
run_off, scan_off, tb, n_msg = w.run_off, w.scan_off, w.tb, w.n_msg
d_world, d_out, d_ref = (g.device_malloc(16 * n_pts) for _ in range(3))
file_off, _ = binding.pcd_file_offsets(run_off, scan_off, K)
F = len(file_off) - 1

timer = rw.EventTimer(g, args)
timed = timer.timed
last = {}


def replay():
    g.batch_replay_runs_cloud_dev(d_pts, run_off, scan_off, tb, 1, n_msg, d_imu, want_poses=False, d_world=d_world)


def downsample():
    last["out_off"], _ = g.downsample_clouds_dev(d_world, file_off, args.leaf, d_out)


def chain():
    return dict(replay=both(timed(replay, before=lambda: g.batch_set_priors(x_run, P_run))), downsample=both(timed(downsample)))


before = chain()
out_off = last["out_off"].copy()
n_map = int(out_off[-1])
ref_off, _ = g.downsample_clouds_dev(d_out, np.array([0, out_off[min(args.ref_files, F)]], dtype=np.uint64), args.leaf, d_ref)
n_ref = int(ref_off[-1])
acc_pairs = [(f, 0) for f in range(F)]
comp_pairs = [(0, f) for f in range(F)]
LAUNCHES = ("c2c_init", "c2c_bounds", "c2c_grid", "c2c_keys", "c2c_gather", "c2c_query", "c2c_reduce")

forms = {}
for md in [float(v) for v in args.max_dist.split(",")]:
    thr = (md / 4, md / 2, md)
    for name, call_args in (("accuracy", (d_out, out_off, d_ref, ref_off, acc_pairs)), ("completeness", (d_ref, ref_off, d_out, out_off, comp_pairs))):
        def call():
            last[name] = g.clouds_c2c_dev(*call_args, md, thr)[0]

        res = timed(call)
        per = rw.per_launch(g, call, LAUNCHES, args.reps)
        rec = last[name]
        build = [sum(per[k][i] for k in LAUNCHES[:5]) for i in range(args.reps)]
        forms[f"{name}_{md:g}"] = dict(max_dist=md, thr=thr, pairs=F, query_points=int(rec["n_query"].sum()), reference_points=n_ref if name == "accuracy" else n_map,
                                       matched=int(rec["n_matched"].sum()), within=[int(v) for v in rec["n_within"].sum(axis=0)[:3]], bad_pairs=int((rec["status"] != 0).sum()),
                                       **both(res), grid_build_launches_ms=stats(build), query_launch_ms=stats(per["c2c_query"]), reduce_launch_ms=stats(per["c2c_reduce"]),
                                       ns_per_query_point=float(np.median(per["c2c_query"])) * 1e6 / max(1, int(rec["n_query"].sum())))
    p, r_, f_ = zip(*(cloudmetrics.fscore(last["accuracy"][f], last["completeness"][f], 1) for f in range(F)))
    forms[f"fscore_{md:g}"] = dict(threshold=md / 2, precision_mean=float(np.mean(p)), recall_mean=float(np.mean(r_)), f_mean=float(np.mean(f_)))
    last[md] = (last["accuracy"].copy(), last["completeness"].copy())

# ---- the parent commit's route: the clouds over PCIe, then a tree per reference cloud on the host
maps, survey = np.zeros((n_map, 4), dtype=np.float32), np.zeros((n_ref, 4), dtype=np.float32)


def fetch():
    g.d2h(maps, d_out)
    g.d2h(survey, d_ref)


baseline = dict(d2h=dict(bytes=int(maps.nbytes + survey.nbytes), **both(timed(fetch))))
nf = min(args.host_files, F)
md0 = float(args.max_dist.split(",")[0])
s64 = survey[:, :3].astype(np.float64)
host, t1 = [], time.perf_counter()
if cKDTree is not None:
    tree = cKDTree(s64)
    for f in range(nf):
        m64 = maps[int(out_off[f]):int(out_off[f + 1]), :3].astype(np.float64)
        da, _ = tree.query(m64, distance_upper_bound=md0)
        dc, _ = cKDTree(m64).query(s64, distance_upper_bound=md0)
        host.append((int(np.isfinite(da).sum()), int(np.isfinite(dc).sum())))
else:
    for f in range(nf):
        m = maps[int(out_off[f]):int(out_off[f + 1])]
        host.append((cloudmetrics.c2c(m, survey, md0)["n_matched"], cloudmetrics.c2c(survey, m, md0)["n_matched"]))
host_s = time.perf_counter() - t1
share = float(out_off[nf]) / n_map
acc, comp = last[md0]
# (a k-d tree decides on sqrt(d2) in another order of operations: a point within 1e-9 of the reach may fall on the other side)
off_by = max(max(abs(int(acc[f]["n_matched"]) - host[f][0]), abs(int(comp[f]["n_matched"]) - host[f][1])) for f in range(nf))

baseline["host"] = dict(method="scipy.spatial.cKDTree" if cKDTree is not None else "legkilo_amd.cloudmetrics.c2c (brute force)", files=nf, max_dist=md0, both_directions=True,
                        wall_ms_measured=host_s * 1e3, points_share=share, wall_ms_all_files_scaled=host_s * 1e3 / share, matched_counts_off_by_at_most=off_by)
after = chain()

print(f"{R} runs x {K} config-1 scans, {n_pts} registered points -> {F} map clouds of {n_map} points (leaf {args.leaf}), survey of {n_ref} points")
for name, v in forms.items():
    if "pairs" in v:
        print(f"  {name:18s}: {v['event_ms']['median']:8.3f} ms between events ({v['event_ms']['min']:.3f} .. {v['event_ms']['max']:.3f}), wall {v['wall_ms']['median']:.3f}; "
              f"build launches {v['grid_build_launches_ms']['median']:.3f}, query {v['query_launch_ms']['median']:.3f}, reduce {v['reduce_launch_ms']['median']:.3f} ms; "
              f"{v['query_points']} query points, {v['matched']} matched, {v['ns_per_query_point']:.3f} ns per query point")
    else:
        print(f"  {name:18s}: precision {v['precision_mean']:.3f}, recall {v['recall_mean']:.3f}, F {v['f_mean']:.3f} at {v['threshold']:g} m")
print(f"  baseline: d2h {baseline['d2h']['wall_ms']['median']:.3f} ms for {baseline['d2h']['bytes']} bytes + {baseline['host']['method']} {baseline['host']['wall_ms_measured']:.0f} ms "
      f"for {nf} files, {baseline['host']['wall_ms_all_files_scaled']:.0f} ms scaled to all files")
for k in ("replay", "downsample"):
    print(f"  {k:10s}: before {before[k]['event_ms']['median']:.3f} ms ({before[k]['event_ms']['min']:.3f} .. {before[k]['event_ms']['max']:.3f}), "
          f"after {after[k]['event_ms']['median']:.3f} ms ({after[k]['event_ms']['min']:.3f} .. {after[k]['event_ms']['max']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/map_c2c.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, leaf=args.leaf,
                       reps=args.reps, warmup=args.warmup, registered_points=n_pts, map_clouds=F, map_points=n_map, survey_points=n_ref, ref_files=args.ref_files,
                       forms=forms, baseline=baseline, chain_before=before, chain_after=after), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_world, d_out, d_ref)
