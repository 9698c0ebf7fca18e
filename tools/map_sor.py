#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what removing the outliers of map clouds costs where they lie (lk_clouds_sor_dev: fewer
than k neighbours within a reach, or a mean distance to the k nearest above mu + n_sigma * sigma of the cloud), on the workload of
tools/runs_workload.py as tools/map_mme.py uses it - R runs of K consecutive config-1 scans replayed on the frozen map with d_world_out, cut into
one file per run and downsampled (lk_downsample_clouds_dev); its d_out / out_off are the map clouds and stay in HBM.  One call filters all of them,
for every k of --k at every reach of --reach, with d_out, d_src_idx and d_keep asked for.
ms per call: median over --reps timed calls after --warmup untimed ones, with min .. max, between two HIP events on the handle's stream and by the
host's wall clock; then, in profiling mode (every launch between its own events), the grid build (bounds, grid, keys, gather - the sort is not a
launch of the library's and is the remainder), the point kernel, the statistics, the flags, the scan, the offsets and the scatter on their own.
lk_clouds_mme_dev runs at the same radius in the same session: it makes the same walk, so the difference of the two point kernels is the price of
the list.  With --one-cloud REACH the same records are also filtered as ONE cloud, once, at the first k (its statistics then fall to one block).
Baseline, the only route the parent commit has: lk_memcpy_d2h of the map clouds, then scipy.spatial.cKDTree.query(k + 1, distance_upper_bound=reach)
per file and numpy on the host (wall clock, over the first --host-files files, scaled by points), then lk_memcpy_h2d of the kept points; the keep
masks of those files are compared with the device's and the number of points that differ is recorded (the tree decides on distances, not on d2).
What the filter does to the scores: MME and MPV (lk_clouds_mme_dev at the reach) and the C2C maximum against the reference cloud of
tools/map_mme.py, on the clouds before and after.
The run replay, lk_downsample_clouds_dev, the C2C accuracy pass at 0.25 m, lk_clouds_mme_dev at 0.3 m and one lk_clouds_align_plane_dev call are
timed before and after the filter calls.
Usage: map_sor.py [--runs R] [--scans K] [--distinct D] [--leaf M] [--k LIST] [--reach LIST] [--n-sigma S] [--reps N] [--warmup W] [--host-files F]
                  [--one-cloud REACH] [--commit TEXT] [--json PATH]"""
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
ap.add_argument("--k", default="8,32")
ap.add_argument("--reach", default="0.3,0.5")
ap.add_argument("--n-sigma", type=float, default=2.0)
ap.add_argument("--ref-files", type=int, default=8, help="map clouds whose union, downsampled once more, is the C2C pass's reference cloud")
ap.add_argument("--host-files", type=int, default=16, help="files of the host baseline")
ap.add_argument("--one-cloud", type=float, default=0.0, metavar="REACH",
                help="also filter all records as ONE cloud at this reach (the clouds lie on top of each other: keep it near leaf / 5) and the first k")
args = ap.parse_args()
HAS_SOR = hasattr(binding.LegKiloHip, "clouds_sor_dev")   # (the tool also times the untouched paths on a library without the entry)

w = rw.Workload(args)
R, K, D, g, d_pts, d_imu, n_pts, x_run, P_run = w.R, w.K, w.D, w.g, w.d_pts, w.d_imu, w.n_pts, w.x, w.P
run_off, scan_off, tb, n_msg = w.run_off, w.scan_off, w.tb, w.n_msg
d_world, d_out, d_ref, d_kept, d_nrm = (g.device_malloc(16 * n_pts) for _ in range(5))
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
    last["c2c"], _ = g.clouds_c2c_dev(d_out, last["out_off"], d_ref, last["ref_off"], [(f, 0) for f in range(F)], 0.25, (0.0625, 0.125, 0.25))


def mme_03():
    g.clouds_mme_dev(d_out, last["out_off"], 0.3, 5)


def plane():
    g.clouds_align_plane_dev(d_out, last["out_off"], d_ref, last["ref_off"], d_nrm, [(f, 0) for f in range(min(F, 64))], 0.25, None, 5, 1e-6, 1e-6)


def chain():
    out = dict(replay=both(timed(replay, before=lambda: g.batch_set_priors(x_run, P_run))), downsample=both(timed(downsample)))
    last["ref_off"], _ = g.downsample_clouds_dev(d_out, np.array([0, last["out_off"][min(args.ref_files, F)]], dtype=np.uint64), args.leaf, d_ref)
    g.clouds_normals_dev(d_ref, last["ref_off"], 0.4, d_nrm, 5, 0.2)
    out["c2c_accuracy_0.25"] = both(timed(accuracy))
    out["mme_0.3"] = both(timed(mme_03))
    out["align_plane_64_pairs_5_iterations"] = both(timed(plane))
    return out


before = chain()
out_off = last["out_off"].copy()
n_map = int(out_off[-1])
d_src, d_keep = g.device_malloc(4 * n_map), g.device_malloc(n_map)
BUILD = ("c2c_init", "c2c_bounds", "c2c_grid", "c2c_keys", "c2c_gather")
OWN = ("sor_point", "sor_stats", "sor_flag", "sor_scan", "sor_offsets", "sor_scatter")
ks = [int(v) for v in args.k.split(",")] if HAS_SOR else []
reaches = [float(v) for v in args.reach.split(",")] if HAS_SOR else []

maps = np.zeros((n_map, 4), dtype=np.float32)
baseline = dict(d2h=dict(bytes=int(maps.nbytes), **both(timed(lambda: g.d2h(maps, d_out)))))
nf = min(args.host_files, F)
share = float(out_off[nf]) / n_map


def host_filter(p64, k, reach, n_sigma):
    """keep mask of one file: the k nearest within reach from a k-d tree, the statistics by numpy"""
    d, _ = cKDTree(p64).query(p64, k + 1, distance_upper_bound=reach)
    d = d[:, 1:]                                               # (the point itself comes first, at 0)
    ok = np.isfinite(d).all(axis=1)
    dbar = np.where(ok, np.where(np.isfinite(d), d, 0.0).sum(axis=1) / k, np.nan)
    if not ok.any():
        return ok
    mu, sigma = dbar[ok].mean(), (dbar[ok].std(ddof=1) if ok.sum() > 1 else 0.0)
    with np.errstate(invalid="ignore"):
        return ok & (dbar <= mu + n_sigma * sigma)


def scores(clouds, off, reach):
    m = g.clouds_mme_dev(clouds, off, reach, 5)
    c, _ = g.clouds_c2c_dev(clouds, off, d_ref, last["ref_off"], [(f, 0) for f in range(F)], 1.0)
    over = lambda v, f=np.mean: float(f(v[~np.isnan(v)])) if (~np.isnan(v)).any() else float("nan")   # noqa: E731  (a filter that kept nothing leaves no figure)
    return dict(mme_mean=over(m["mme"]), mpv_mean=over(m["mpv"]), c2c_max_mean=over(c["max"]), c2c_max_max=over(c["max"], np.max), c2c_rmse_mean=over(c["rmse"]))


forms = {}
for reach in reaches:
    def mme_call():
        last["mme"] = g.clouds_mme_dev(d_out, out_off, reach, 5)

    mme_res = timed(mme_call)
    mme_per = rw.per_launch(g, mme_call, BUILD + ("mme_point", "mme_reduce"), args.reps)
    unfiltered = scores(d_out, out_off, reach)
    for k in ks:
        def call():
            last["sor"], last["kept_off"] = g.clouds_sor_dev(d_out, out_off, k, reach, args.n_sigma, d_kept, d_src, d_keep)

        res = timed(call)
        per = rw.per_launch(g, call, BUILD + OWN, args.reps)
        rec, kept_off = last["sor"], last["kept_off"].copy()
        build = [sum(per[b][i] for b in BUILD) for i in range(args.reps)]
        n_kept = int(kept_off[-1])
        host = None
        if cKDTree is not None:
            keep = np.zeros(n_map, dtype=np.uint8)
            g.d2h(keep, d_keep)
            t1, differ = time.perf_counter(), 0
            masks = [host_filter(maps[int(out_off[f]):int(out_off[f + 1]), :3].astype(np.float64), k, reach, args.n_sigma) for f in range(nf)]
            host_s = time.perf_counter() - t1
            for f in range(nf):
                differ += int((masks[f] != keep[int(out_off[f]):int(out_off[f + 1])].astype(bool)).sum())
            up = both(timed(lambda: g.h2d(d_world, maps[:max(n_kept, 1)])))   # (d_world is free between the chains)
            host = dict(method="scipy.spatial.cKDTree.query(k + 1, distance_upper_bound=reach) + numpy", files=nf, wall_ms_measured=host_s * 1e3, points_share=share,
                        wall_ms_all_files_scaled=host_s * 1e3 / share, keep_differs_in_points=differ, points_of_those_files=int(out_off[nf]), upload_of_the_kept_points=up)
        one = None
        if args.one_cloud > 0.0 and k == ks[0] and reach == reaches[0]:
            def call_one():
                last["one"], _ = g.clouds_sor_dev(d_out, np.array([0, n_map], dtype=np.uint64), k, args.one_cloud, args.n_sigma, d_kept, d_src, d_keep)

            one_res = timed(call_one)
            one_per = rw.per_launch(g, call_one, ("sor_point", "sor_stats"), args.reps)
            one = dict(reach=args.one_cloud, **both(one_res), point_launch_ms=stats(one_per["sor_point"]), stats_launch_ms=stats(one_per["sor_stats"]), kept=int(last["one"][0]["n_kept"]))
            call()                                                            # d_kept holds the per-cloud result again
        forms[f"sor_k{k}_{reach:g}"] = dict(
            k=k, reach=reach, n_sigma=args.n_sigma, clouds=F, points=int(rec["n_points"].sum()), isolated=int(rec["n_isolated"].sum()), outliers=int(rec["n_outliers"].sum()),
            kept=n_kept, bad_clouds=int((rec["status"] != 0).sum()), share_isolated=float(rec["n_isolated"].sum()) / n_map, share_outliers=float(rec["n_outliers"].sum()) / n_map,
            neighbours_per_point=float(last["mme"]["n_pairs"].sum()) / n_map - 1.0, **both(res), grid_build_launches_ms=stats(build),
            **{name[4:] + "_launch_ms": stats(per[name]) for name in OWN}, ns_per_point=float(np.median(per["sor_point"])) * 1e6 / n_map,
            mme_same_radius=dict(**both(mme_res), point_launch_ms=stats(mme_per["mme_point"]), reduce_launch_ms=stats(mme_per["mme_reduce"])),
            point_kernel_over_mme=float(np.median(per["sor_point"])) / float(np.median(mme_per["mme_point"])),
            scores_unfiltered=unfiltered, scores_filtered=scores(d_kept, kept_off, reach), host_baseline=host, one_cloud=one)
after = chain()

print(f"{R} runs x {K} config-1 scans, {n_pts} registered points -> {F} map clouds of {n_map} points (leaf {args.leaf})")
for name, v in forms.items():
    print(f"  {name:12s}: {v['event_ms']['median']:8.3f} ms between events ({v['event_ms']['min']:.3f} .. {v['event_ms']['max']:.3f}), wall {v['wall_ms']['median']:.3f}; "
          f"build launches {v['grid_build_launches_ms']['median']:.3f}, point {v['point_launch_ms']['median']:.3f}, stats {v['stats_launch_ms']['median']:.3f}, "
          f"flag {v['flag_launch_ms']['median']:.3f}, scan {v['scan_launch_ms']['median']:.3f}, offsets {v['offsets_launch_ms']['median']:.3f}, "
          f"scatter {v['scatter_launch_ms']['median']:.3f} ms; mme at the radius {v['mme_same_radius']['event_ms']['median']:.3f} ms, its point kernel "
          f"{v['mme_same_radius']['point_launch_ms']['median']:.3f} ms (x {v['point_kernel_over_mme']:.2f}); {v['neighbours_per_point']:.1f} neighbours per point; isolated "
          f"{100 * v['share_isolated']:.2f} %, outliers {100 * v['share_outliers']:.2f} %")
    print(f"    scores: {v['scores_unfiltered']} -> {v['scores_filtered']}")
    if v["host_baseline"]:
        hb = v["host_baseline"]
        print(f"    baseline: d2h {baseline['d2h']['wall_ms']['median']:.3f} ms + {hb['method']} {hb['wall_ms_measured']:.0f} ms for {nf} files, "
              f"{hb['wall_ms_all_files_scaled']:.0f} ms scaled to all files + upload {hb['upload_of_the_kept_points']['wall_ms']['median']:.3f} ms; keep differs in "
              f"{hb['keep_differs_in_points']} of {hb['points_of_those_files']} points")
    if v["one_cloud"]:
        oc = v["one_cloud"]
        print(f"    as one cloud: {oc['event_ms']['median']:.3f} ms, point {oc['point_launch_ms']['median']:.3f}, stats {oc['stats_launch_ms']['median']:.3f} ms")
for key in before:
    print(f"  {key:34s}: before {before[key]['event_ms']['median']:.3f} ms ({before[key]['event_ms']['min']:.3f} .. {before[key]['event_ms']['max']:.3f}), "
          f"after {after[key]['event_ms']['median']:.3f} ms ({after[key]['event_ms']['min']:.3f} .. {after[key]['event_ms']['max']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/map_sor.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, leaf=args.leaf,
                       reps=args.reps, warmup=args.warmup, registered_points=n_pts, map_clouds=F, map_points=n_map, forms=forms, baseline=baseline,
                       chain_before=before, chain_after=after), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_world, d_out, d_ref, d_kept, d_nrm, d_src, d_keep)
