#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what scoring map clouds WITHOUT a reference costs (lk_clouds_mme_dev: mean map entropy and
mean plane variance), on the workload of tools/runs_workload.py as tools/map_c2c.py uses it - R runs of K consecutive config-1 scans replayed on the
frozen map with d_world_out, cut into one file per run and downsampled (lk_downsample_clouds_dev); its d_out / out_off are the map clouds and stay in
HBM.  One call scores all of them, at every radius of --radius.
ms per call: median over --reps timed calls after --warmup untimed ones, with min .. max, between two HIP events on the handle's stream (the call is
synchronous, the events bracket it) and by the host's wall clock; then, in profiling mode (every launch between its own events), the grid build
(bounds, grid, keys, gather - the sort is not a launch of the library's and is the remainder), the point kernel and the reduce on their own.
Neighbours per point come from the records (n_pairs / n_points); records looked at per point - the records of the 27 cells around a point's own - are
counted on the host over the first --host-files files, and the rate of distance evaluations is that count scaled to all points over the point
kernel's time.
Baseline, the only route the parent commit has: lk_memcpy_d2h of the map clouds, then scipy.spatial.cKDTree.query_pairs per file and the second moments
by numpy on the host (wall clock, over the first --host-files files, scaled by points); n_pairs of those files is compared with the device's and the
largest difference is recorded (the tree decides on distances, not on d2).
The run replay, lk_downsample_clouds_dev and the C2C accuracy pass at 0.25 m are timed before and after the MME calls (tools/runs_cloud.py's,
tools/map_clouds.py's and tools/map_c2c.py's figures).
Usage: map_mme.py [--runs R] [--scans K] [--distinct D] [--leaf M] [--radius LIST] [--min-pts N] [--reps N] [--warmup W] [--host-files F] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding, both, stats

try:
    from scipy.spatial import cKDTree
except ImportError:
    cKDTree = None

ap = rw.parser()
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--radius", default="0.3,0.5")
ap.add_argument("--min-pts", type=int, default=5)
ap.add_argument("--ref-files", type=int, default=8, help="map clouds whose union, downsampled once more, is the C2C pass's reference cloud")
ap.add_argument("--host-files", type=int, default=16, help="files of the host baseline")
args = ap.parse_args()
HAS_MME = hasattr(binding.LegKiloHip, "clouds_mme_dev")   # (the tool also times the untouched paths on a library without the entry)

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


def accuracy():
    g.clouds_c2c_dev(d_out, last["out_off"], d_ref, last["ref_off"], [(f, 0) for f in range(F)], 0.25, (0.0625, 0.125, 0.25))


def chain():
    out = dict(replay=both(timed(replay, before=lambda: g.batch_set_priors(x_run, P_run))), downsample=both(timed(downsample)))
    last["ref_off"], _ = g.downsample_clouds_dev(d_out, np.array([0, last["out_off"][min(args.ref_files, F)]], dtype=np.uint64), args.leaf, d_ref)
    out["c2c_accuracy_0.25"] = both(timed(accuracy))
    return out


before = chain()
out_off = last["out_off"].copy()
n_map = int(out_off[-1])
BUILD = ("c2c_init", "c2c_bounds", "c2c_grid", "c2c_keys", "c2c_gather")
radii = [float(v) for v in args.radius.split(",")] if HAS_MME else []

maps = np.zeros((n_map, 4), dtype=np.float32)
baseline = dict(d2h=dict(bytes=int(maps.nbytes), **both(timed(lambda: g.d2h(maps, d_out)))))
nf = min(args.host_files, F)
share = float(out_off[nf]) / n_map


def looked_at(p64, edge):
    """records of the 27 cells around each point's own, summed over the points"""
    k = np.floor(p64 / edge).astype(np.int64)
    k -= k.min(0)
    dv = k.max(0) + 3
    key = (k[:, 0] + 1) + dv[0] * ((k[:, 1] + 1) + dv[1] * (k[:, 2] + 1))
    cells, counts = np.unique(key, return_counts=True)
    total = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = key + dx + dv[0] * (dy + dv[1] * dz)
                at = np.minimum(np.searchsorted(cells, q), len(cells) - 1)
                total += int(counts[at][cells[at] == q].sum())
    return total


def host_moments(p64, radius):
    """n_pairs of a file, and the nine sums per point (what the figures are made of), the neighbours from a k-d tree"""
    pairs = cKDTree(p64).query_pairs(radius, output_type="ndarray")
    i, j = np.r_[pairs[:, 0], pairs[:, 1]], np.r_[pairs[:, 1], pairs[:, 0]]
    u = p64[j] - p64[i]
    m = len(p64)
    n = np.bincount(i, minlength=m) + 1
    sums = [np.bincount(i, weights=u[:, a], minlength=m) for a in range(3)]
    sums += [np.bincount(i, weights=u[:, a] * u[:, b], minlength=m) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return int(n.sum()), sums


forms = {}
for radius in radii:
    def call():
        last["mme"] = g.clouds_mme_dev(d_out, out_off, radius, args.min_pts)

    res = timed(call)
    per = rw.per_launch(g, call, BUILD + ("mme_point", "mme_reduce"), args.reps)
    rec = last["mme"]
    build = [sum(per[k][i] for k in BUILD) for i in range(args.reps)]
    seen = sum(looked_at(maps[int(out_off[f]):int(out_off[f + 1]), :3].astype(np.float64), radius) for f in range(nf))
    point_ms = float(np.median(per["mme_point"]))
    host = None
    if cKDTree is not None:
        t1, host_pairs = time.perf_counter(), []
        for f in range(nf):
            host_pairs.append(host_moments(maps[int(out_off[f]):int(out_off[f + 1]), :3].astype(np.float64), radius)[0])
        host_s = time.perf_counter() - t1
        off_by = max(abs(int(rec[f]["n_pairs"]) - host_pairs[f]) for f in range(nf))
        host = dict(method="scipy.spatial.cKDTree.query_pairs + numpy bincount of the nine sums", files=nf, wall_ms_measured=host_s * 1e3, points_share=share,
                    wall_ms_all_files_scaled=host_s * 1e3 / share, n_pairs_off_by_at_most=off_by, n_pairs_of_those_files=int(sum(host_pairs)))
    forms[f"mme_{radius:g}"] = dict(radius=radius, min_pts=args.min_pts, clouds=F, points=int(rec["n_points"].sum()), dense=int(rec["n_dense"].sum()),
                                    scored=int(rec["n_scored"].sum()), bad_clouds=int((rec["status"] != 0).sum()), mme_mean=float(np.nanmean(rec["mme"])),
                                    mpv_mean=float(np.nanmean(rec["mpv"])), neighbours_per_point=float(rec["n_pairs"].sum()) / n_map,
                                    records_looked_at_per_point=seen / float(out_off[nf]), **both(res), grid_build_launches_ms=stats(build),
                                    point_launch_ms=stats(per["mme_point"]), reduce_launch_ms=stats(per["mme_reduce"]),
                                    distance_evaluations_per_s=seen / share / (point_ms * 1e-3), ns_per_point=point_ms * 1e6 / n_map, host_baseline=host)
after = chain()

print(f"{R} runs x {K} config-1 scans, {n_pts} registered points -> {F} map clouds of {n_map} points (leaf {args.leaf})")
for name, v in forms.items():
    print(f"  {name:10s}: {v['event_ms']['median']:8.3f} ms between events ({v['event_ms']['min']:.3f} .. {v['event_ms']['max']:.3f}), wall {v['wall_ms']['median']:.3f}; "
          f"build launches {v['grid_build_launches_ms']['median']:.3f}, point kernel {v['point_launch_ms']['median']:.3f}, reduce {v['reduce_launch_ms']['median']:.3f} ms; "
          f"{v['neighbours_per_point']:.1f} neighbours and {v['records_looked_at_per_point']:.1f} records looked at per point, "
          f"{v['distance_evaluations_per_s'] / 1e9:.1f} G distance evaluations / s; dense {v['dense']}, scored {v['scored']}, mme {v['mme_mean']:.4f}, mpv {v['mpv_mean']:.3e}")
    if v["host_baseline"]:
        hb = v["host_baseline"]
        print(f"    baseline: d2h {baseline['d2h']['wall_ms']['median']:.3f} ms for {baseline['d2h']['bytes']} bytes + {hb['method']} {hb['wall_ms_measured']:.0f} ms for "
              f"{nf} files, {hb['wall_ms_all_files_scaled']:.0f} ms scaled to all files; n_pairs off by at most {hb['n_pairs_off_by_at_most']}")
for k in before:
    print(f"  {k:18s}: before {before[k]['event_ms']['median']:.3f} ms ({before[k]['event_ms']['min']:.3f} .. {before[k]['event_ms']['max']:.3f}), "
          f"after {after[k]['event_ms']['median']:.3f} ms ({after[k]['event_ms']['min']:.3f} .. {after[k]['event_ms']['max']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/map_mme.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, leaf=args.leaf,
                       reps=args.reps, warmup=args.warmup, registered_points=n_pts, map_clouds=F, map_points=n_map, forms=forms, baseline=baseline,
                       chain_before=before, chain_after=after), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_world, d_out, d_ref)
