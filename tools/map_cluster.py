#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what clustering map clouds costs where they lie (lk_clouds_cluster_dev: DBSCAN, with
min_pts 1 the connected components within a reach), on the workload of tools/runs_workload.py as tools/map_sor.py uses it - R runs of K consecutive
config-1 scans replayed on the frozen map with d_world_out, cut into one file per run and downsampled (lk_downsample_clouds_dev); its d_out / out_off
are the map clouds and stay in HBM.  One call clusters all of them, for every min_pts of --min-pts at every reach of --reach, with LK_CLUSTER_KEEP_LARGEST
and d_label, d_kind, d_cl_size, d_out and d_src_idx asked for.
ms per call: median over --reps timed calls after --warmup untimed ones, with min .. max, between two HIP events on the handle's stream and by the
host's wall clock; then, in profiling mode (every launch between its own events), the grid build (bounds, grid, keys, gather - the sort is not a
launch of the library's and is the remainder) and every kernel of the route on its own.  lk_clouds_mme_dev and lk_clouds_sor_dev (k 8) run at the
same radius in the same session: the route walks three times where they walk once.  With --one-cloud REACH the same records are also clustered as
ONE cloud at min_pts 1 (its record then falls to one block, and every union of the call works on one cloud's parents).
Baseline, the only route the parent commit has: lk_memcpy_d2h of the map clouds, then per file scipy.spatial.cKDTree.query_pairs and
scipy.sparse.csgraph.connected_components (min_pts 1) or sklearn.cluster.DBSCAN (min_pts above 1) on the host (wall clock, over the first
--host-files files, scaled by points), then lk_memcpy_h2d of the kept points.  The labels of those files are compared with the device's: the core
set, the noise set and the labels of the core points after renumbering the host's clusters by their smallest core index must be equal; border points
that a first-visit rule puts elsewhere are counted.
The run replay, lk_downsample_clouds_dev, the C2C accuracy pass at 0.25 m, lk_clouds_mme_dev at 0.3 m and lk_clouds_sor_dev (k 8, 0.3 m) are timed
before and after the clustering calls.
Usage: map_cluster.py [--runs R] [--scans K] [--distinct D] [--leaf M] [--min-pts LIST] [--reach LIST] [--reps N] [--warmup W] [--host-files F]
                      [--one-cloud REACH] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding, both, stats

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    from sklearn.cluster import DBSCAN
except ImportError:
    cKDTree = None

ap = rw.parser()
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--min-pts", default="1,8")
ap.add_argument("--reach", default="0.3,0.5")
ap.add_argument("--ref-files", type=int, default=8, help="map clouds whose union, downsampled once more, is the C2C pass's reference cloud")
ap.add_argument("--host-files", type=int, default=16, help="files of the host baseline")
ap.add_argument("--one-cloud", type=float, default=0.0, metavar="REACH",
                help="also cluster all records as ONE cloud at this reach (the clouds lie on top of each other: keep it near leaf / 5) and min_pts 1")
args = ap.parse_args()
HAS = hasattr(binding.LegKiloHip, "clouds_cluster_dev")   # (the tool also times the untouched paths on a library without the entry)

w = rw.Workload(args)
R, K, D, g, d_pts, d_imu, n_pts, x_run, P_run = w.R, w.K, w.D, w.g, w.d_pts, w.d_imu, w.n_pts, w.x, w.P
run_off, scan_off, tb, n_msg = w.run_off, w.scan_off, w.tb, w.n_msg
d_world, d_out, d_ref, d_kept = (g.device_malloc(16 * n_pts) for _ in range(4))
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


def sor_03():
    g.clouds_sor_dev(d_out, last["out_off"], 8, 0.3, 2.0, want_off=True)


def chain():
    out = dict(replay=both(timed(replay, before=lambda: g.batch_set_priors(x_run, P_run))), downsample=both(timed(downsample)))
    last["ref_off"], _ = g.downsample_clouds_dev(d_out, np.array([0, last["out_off"][min(args.ref_files, F)]], dtype=np.uint64), args.leaf, d_ref)
    out["c2c_accuracy_0.25"] = both(timed(accuracy))
    out["mme_0.3"] = both(timed(mme_03))
    out["sor_k8_0.3"] = both(timed(sor_03))
    return out


before = chain()
out_off = last["out_off"].copy()
n_map = int(out_off[-1])
d_label, d_kind, d_size, d_src = g.device_malloc(4 * n_map), g.device_malloc(n_map), g.device_malloc(4 * n_map), g.device_malloc(4 * n_map)
BUILD = ("c2c_init", "c2c_bounds", "c2c_grid", "c2c_keys", "c2c_gather")
OWN = ("cluster_count", "cluster_link", "cluster_assign", "cluster_rootflag", "cluster_ids", "cluster_label", "cluster_record", "cluster_tables", "cluster_flag",
       "cluster_scan", "cluster_offsets", "cluster_scatter")
WALKS = OWN[:3]
mps = [int(v) for v in args.min_pts.split(",")] if HAS else []
reaches = [float(v) for v in args.reach.split(",")] if HAS else []
LARGEST = 1

maps = np.zeros((n_map, 4), dtype=np.float32)
baseline = dict(d2h=dict(bytes=int(maps.nbytes), **both(timed(lambda: g.d2h(maps, d_out)))))
nf = min(args.host_files, F)
share = float(out_off[nf]) / n_map


def host_cluster(p64, reach, min_pts):
    """(label int64, -1 = noise; core bool) of one file on the host"""
    if min_pts == 1:
        pairs = cKDTree(p64).query_pairs(reach, output_type="ndarray")
        _, lab = connected_components(coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(p64), len(p64))), directed=False)
        return lab.astype(np.int64), np.ones(len(p64), dtype=bool)
    db = DBSCAN(eps=reach, min_samples=min_pts, algorithm="kd_tree").fit(p64)
    core = np.zeros(len(p64), dtype=bool)
    core[db.core_sample_indices_] = True
    return db.labels_.astype(np.int64), core


def by_first_core(lab, core):
    """the labels with the clusters renumbered in ascending order of their smallest core index (noise stays -1)"""
    ids, first = np.unique(lab[core], return_index=True)
    rank = np.full(int(lab.max()) + 2, -1, dtype=np.int64)
    rank[ids[np.argsort(first, kind="stable")]] = np.arange(len(ids))
    return np.where(lab >= 0, rank[lab], -1)


forms = {}
for reach in reaches:
    def mme_call():
        last["mme"] = g.clouds_mme_dev(d_out, out_off, reach, 5)

    def sor_call():
        g.clouds_sor_dev(d_out, out_off, 8, reach, 2.0, d_kept, d_src)

    mme_res, sor_res = timed(mme_call), timed(sor_call)
    mme_per = rw.per_launch(g, mme_call, BUILD + ("mme_point", "mme_reduce"), args.reps)
    sor_per = rw.per_launch(g, sor_call, ("sor_point",), args.reps)
    for mp in mps:
        def call():
            last["res"], last["cl_off"], last["kept_off"] = g.clouds_cluster_dev(d_out, out_off, reach, mp, 0, 0xFFFFFFFF, LARGEST, d_label, d_kind, 0, d_size, 0, d_kept, d_src)

        res = timed(call)
        per = rw.per_launch(g, call, BUILD + OWN, args.reps)
        rec, kept_off = last["res"], last["kept_off"].copy()
        build = [sum(per[b][i] for b in BUILD) for i in range(args.reps)]
        walks = [sum(per[b][i] for b in WALKS) for i in range(args.reps)]
        n_kept = int(kept_off[-1])
        host = None
        if cKDTree is not None:
            label, kind = np.zeros(n_map, dtype=np.uint32), np.zeros(n_map, dtype=np.uint8)
            g.d2h(label, d_label), g.d2h(kind, d_kind)
            t1 = time.perf_counter()
            got = [host_cluster(maps[int(out_off[f]):int(out_off[f + 1]), :3].astype(np.float64), reach, mp) for f in range(nf)]
            host_s = time.perf_counter() - t1
            core_differs = noise_differs = core_label_differs = border_elsewhere = 0
            for f, (lab, core) in enumerate(got):
                a, b = int(out_off[f]), int(out_off[f + 1])
                dl, dk = label[a:b].astype(np.int64), kind[a:b]
                dl[dl == 0xFFFFFFFF] = -1
                hl = by_first_core(lab, core)
                core_differs += int((core != (dk == 2)).sum())
                noise_differs += int(((lab < 0) != (dk == 0)).sum())
                core_label_differs += int((hl[core] != dl[core]).sum())
                border_elsewhere += int((hl[dk == 1] != dl[dk == 1]).sum())
            up = both(timed(lambda: g.h2d(d_world, maps[:max(n_kept, 1)])))   # (d_world is free between the chains)
            host = dict(method="cKDTree.query_pairs + connected_components" if mp == 1 else "sklearn.cluster.DBSCAN(kd_tree)", files=nf, wall_ms_measured=host_s * 1e3,
                        points_share=share, wall_ms_all_files_scaled=host_s * 1e3 / share, points_of_those_files=int(out_off[nf]), core_differs=core_differs,
                        noise_differs=noise_differs, core_label_differs=core_label_differs, border_points_put_elsewhere=border_elsewhere, upload_of_the_kept_points=up)
        one = None
        if args.one_cloud > 0.0 and mp == mps[0] and reach == reaches[0]:
            def call_one():
                last["one"], _, _ = g.clouds_cluster_dev(d_out, np.array([0, n_map], dtype=np.uint64), args.one_cloud, 1, 0, 0xFFFFFFFF, LARGEST, d_label, d_kind, 0, d_size, 0,
                                                         d_kept, d_src)

            one_res = timed(call_one)
            one_per = rw.per_launch(g, call_one, OWN, args.reps)
            one = dict(reach=args.one_cloud, min_pts=1, **both(one_res), **{name[8:] + "_launch_ms": stats(one_per[name]) for name in OWN},
                       clusters=int(last["one"][0]["n_clusters"]), largest_size=int(last["one"][0]["largest_size"]))
            call()                                                            # the arrays hold the per-cloud result again
        m = float(np.median(mme_per["mme_point"]))
        forms[f"cluster_mp{mp}_{reach:g}"] = dict(
            min_pts=mp, reach=reach, flags="LK_CLUSTER_KEEP_LARGEST", clouds=F, points=int(rec["n_points"].sum()), core=int(rec["n_core"].sum()),
            border=int(rec["n_border"].sum()), noise=int(rec["n_noise"].sum()), clusters=int(rec["n_clusters"].sum()), kept=n_kept, bad_clouds=int((rec["status"] != 0).sum()),
            neighbours_per_point=float(last["mme"]["n_pairs"].sum()) / n_map - 1.0, **both(res), grid_build_launches_ms=stats(build), three_walks_ms=stats(walks),
            **{name[8:] + "_launch_ms": stats(per[name]) for name in OWN},
            mme_same_radius=dict(**both(mme_res), point_launch_ms=stats(mme_per["mme_point"]), reduce_launch_ms=stats(mme_per["mme_reduce"])),
            sor_k8_same_radius=dict(**both(sor_res), point_launch_ms=stats(sor_per["sor_point"])),
            call_over_mme_call=float(np.median([a for a, _ in res])) / float(np.median([a for a, _ in mme_res])),
            walks_over_mme_point_kernel=float(np.median(walks)) / m, host_baseline=host, one_cloud=one)
after = chain()

print(f"{R} runs x {K} config-1 scans, {n_pts} registered points -> {F} map clouds of {n_map} points (leaf {args.leaf})")
for name, v in forms.items():
    print(f"  {name:18s}: {v['event_ms']['median']:8.3f} ms between events ({v['event_ms']['min']:.3f} .. {v['event_ms']['max']:.3f}), wall {v['wall_ms']['median']:.3f}; "
          f"build launches {v['grid_build_launches_ms']['median']:.3f}, " + ", ".join(f"{n[8:]} {v[n[8:] + '_launch_ms']['median']:.3f}" for n in OWN)
          + f" ms; mme at the radius {v['mme_same_radius']['event_ms']['median']:.3f} ms, its point kernel {v['mme_same_radius']['point_launch_ms']['median']:.3f} ms; "
          f"sor k 8 {v['sor_k8_same_radius']['event_ms']['median']:.3f} ms; the call x {v['call_over_mme_call']:.2f} mme's, the three walks x {v['walks_over_mme_point_kernel']:.2f} "
          f"its point kernel; {v['neighbours_per_point']:.1f} neighbours per point; core {v['core']}, border {v['border']}, noise {v['noise']}, clusters {v['clusters']}, "
          f"kept {v['kept']}")
    if v["host_baseline"]:
        hb = v["host_baseline"]
        print(f"    baseline: d2h {baseline['d2h']['wall_ms']['median']:.3f} ms + {hb['method']} {hb['wall_ms_measured']:.0f} ms for {nf} files, "
              f"{hb['wall_ms_all_files_scaled']:.0f} ms scaled to all files + upload {hb['upload_of_the_kept_points']['wall_ms']['median']:.3f} ms; of "
              f"{hb['points_of_those_files']} points the core set differs in {hb['core_differs']}, the noise set in {hb['noise_differs']}, the core points' labels in "
              f"{hb['core_label_differs']}; border points put elsewhere {hb['border_points_put_elsewhere']}")
    if v["one_cloud"]:
        oc = v["one_cloud"]
        print(f"    as one cloud at reach {oc['reach']}: {oc['event_ms']['median']:.3f} ms; " + ", ".join(f"{n[8:]} {oc[n[8:] + '_launch_ms']['median']:.3f}" for n in OWN)
              + f"; {oc['clusters']} clusters, the largest {oc['largest_size']}")
for key in before:
    print(f"  {key:34s}: before {before[key]['event_ms']['median']:.3f} ms ({before[key]['event_ms']['min']:.3f} .. {before[key]['event_ms']['max']:.3f}), "
          f"after {after[key]['event_ms']['median']:.3f} ms ({after[key]['event_ms']['min']:.3f} .. {after[key]['event_ms']['max']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/map_cluster.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, leaf=args.leaf,
                       reps=args.reps, warmup=args.warmup, registered_points=n_pts, map_clouds=F, map_points=n_map, forms=forms, baseline=baseline,
                       chain_before=before, chain_after=after), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_world, d_out, d_ref, d_kept, d_label, d_kind, d_size, d_src)
