#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what peeling the dominant planes off map clouds costs where they lie
(lk_clouds_planes_dev: RANSAC, hypotheses x records of non-fused float64), on the workload of tools/runs_workload.py as tools/map_cluster.py uses it
- R runs of K consecutive config-1 scans replayed on the frozen map with d_world_out, cut into one file per run and downsampled
(lk_downsample_clouds_dev); its d_out / out_off are the map clouds and stay in HBM.  One call takes all of them, with d_label, d_out and d_src_idx
asked for: at --hyp hypotheses for 1 .. --planes rounds, and at every count of --hyp-list for --planes rounds.
ms per call: median over --reps timed calls after --warmup untimed ones, with min .. max, between two HIP events on the handle's stream and by the
host's wall clock; then, in profiling mode (every launch between its own events), every kernel of the route on its own - for the one-round form that
is the split of a round.  The score kernel's rate: tests = hypotheses x records of the remainders it ran on (from the records the call returns), ten
float64 operations each (three subtractions, three products, two additions, the square, the comparison), against the 78.6 TFLOP/s the data sheet
gives the vector unit with fused multiply-adds - 39.3 T non-fused operations a second.  lk_clouds_mme_dev at r = 0.3 runs in the same session as the
family's yardstick.  With --one-cloud the same records are also taken as ONE cloud.
Baseline, the only route the parent commit has: lk_memcpy_d2h of the map clouds, then cloudmetrics.planes in numpy per file on the host (wall clock,
over the first --host-files files, scaled by points), then lk_memcpy_h2d of the kept points.  The labels of those files must equal the device's.
The run replay, lk_downsample_clouds_dev, the C2C accuracy pass at 0.25 m, lk_clouds_mme_dev at 0.3 m, lk_clouds_sor_dev (k 8, 0.3 m) and
lk_clouds_cluster_dev (min_pts 1, 0.3 m) are timed before and after the new calls.
Usage: map_planes.py [--runs R] [--scans K] [--distinct D] [--leaf M] [--dist M] [--hyp N] [--hyp-list LIST] [--planes P] [--min-inliers N] [--seed S]
                     [--reps N] [--warmup W] [--host-files F] [--one-cloud] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding, both, stats

from legkilo_amd import cloudmetrics

ap = rw.parser()
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--dist", type=float, default=0.05)
ap.add_argument("--hyp", type=int, default=256)
ap.add_argument("--hyp-list", default="64,256,1024")
ap.add_argument("--planes", type=int, default=4)
ap.add_argument("--min-inliers", type=int, default=200)
ap.add_argument("--seed", type=int, default=20261021)
ap.add_argument("--ref-files", type=int, default=8, help="map clouds whose union, downsampled once more, is the C2C pass's reference cloud")
ap.add_argument("--host-files", type=int, default=16, help="files of the host baseline")
ap.add_argument("--one-cloud", action="store_true", help="also take all records as ONE cloud")
args = ap.parse_args()
HAS = hasattr(binding.LegKiloHip, "clouds_planes_dev")   # (the tool also times the untouched paths on a library without the entry)
NONFUSED_FP64_PER_S = 78.6e12 / 2.0
OPS_PER_TEST = 10

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
    last["mme"] = g.clouds_mme_dev(d_out, last["out_off"], 0.3, 5)


def sor_03():
    g.clouds_sor_dev(d_out, last["out_off"], 8, 0.3, 2.0, want_off=True)


def cluster_03():
    g.clouds_cluster_dev(d_out, last["out_off"], 0.3, 1, want_off=True)


def chain():
    out = dict(replay=both(timed(replay, before=lambda: g.batch_set_priors(x_run, P_run))), downsample=both(timed(downsample)))
    last["ref_off"], _ = g.downsample_clouds_dev(d_out, np.array([0, last["out_off"][min(args.ref_files, F)]], dtype=np.uint64), args.leaf, d_ref)
    out["c2c_accuracy_0.25"] = both(timed(accuracy))
    out["mme_0.3"] = both(timed(mme_03))
    out["sor_k8_0.3"] = both(timed(sor_03))
    out["cluster_mp1_0.3"] = both(timed(cluster_03))
    return out


before = chain()
out_off = last["out_off"].copy()
n_map = int(out_off[-1])
d_label, d_src = g.device_malloc(4 * n_map), g.device_malloc(4 * n_map)
OWN = ("c2c_init", "c2c_bounds", "planes_init", "planes_scan", "planes_compact", "planes_score", "planes_argmax", "planes_mark", "planes_refit", "planes_fit", "planes_record", "planes_keep",
       "planes_keep_scan", "planes_offsets", "planes_scatter")

maps = np.zeros((n_map, 4), dtype=np.float32)
baseline = dict(d2h=dict(bytes=int(maps.nbytes), **both(timed(lambda: g.d2h(maps, d_out)))))
nf = min(args.host_files, F)
share = float(out_off[nf]) / n_map


def measure(off, n_hyp, max_planes, host=False):
    def call():
        last["res"], last["planes"], last["kept_off"] = g.clouds_planes_dev(d_out, off, args.dist, n_hyp, max_planes, args.min_inliers, None, 0.0, args.seed, 0, d_label, d_kept,
                                                                            d_src)

    res = timed(call)
    per = rw.per_launch(g, call, OWN, args.reps)
    rec, pl = last["res"], last["planes"]
    n_kept = int(last["kept_off"][-1])
    # records the score kernel tested: per cloud the remainder of every round that ran - a round runs while the one before found a plane
    sizes = rec["n_points"].astype(np.int64)
    took = np.cumsum(pl["n_inliers"].astype(np.int64), axis=1)
    m_r = np.concatenate([sizes[:, None], sizes[:, None] - took[:, :-1]], axis=1)
    ran = np.concatenate([np.ones((len(rec), 1), dtype=bool), pl["n_inliers"][:, :-1] > 0], axis=1) & (m_r >= max(3, args.min_inliers)) & (rec["status"] == 0)[:, None]
    tests = float((m_r * ran).sum()) * n_hyp
    score_ms = float(np.median(per["planes_score"]))
    out = dict(n_hyp=n_hyp, max_planes=max_planes, dist=args.dist, min_inliers=args.min_inliers, clouds=len(rec), points=int(sizes.sum()), planes=int(rec["n_planes"].sum()),
               on_planes=int(rec["n_on_planes"].sum()), rest=int(rec["n_rest"].sum()), kept=n_kept, bad_clouds=int((rec["status"] != 0).sum()),
               planes_per_round=[int((pl["n_inliers"][:, r] > 0).sum()) for r in range(max_planes)],
               mean_rmse=float(pl["rmse"][pl["n_inliers"] > 0].mean()) if (pl["n_inliers"] > 0).any() else None, **both(res),
               **{name + "_launch_ms": stats(per[name]) for name in OWN}, score_tests=tests,
               score_fraction_of_nonfused_fp64_rate=tests * OPS_PER_TEST / (score_ms * 1e-3) / NONFUSED_FP64_PER_S if score_ms > 0 else None)
    if host:
        label = np.zeros(n_map, dtype=np.uint32)
        g.d2h(label, d_label)
        t1 = time.perf_counter()
        got = [cloudmetrics.planes(maps[int(out_off[f]):int(out_off[f + 1]), :3], args.dist, n_hyp, max_planes, args.min_inliers, None, 0.0, args.seed) for f in range(nf)]
        host_s = time.perf_counter() - t1
        differs = sum(int((h["label"] != label[int(out_off[f]):int(out_off[f + 1])]).sum()) for f, h in enumerate(got))
        assert differs == 0, f"{differs} labels of the first {nf} files differ from the numpy statement's"
        up = both(timed(lambda: g.h2d(d_world, maps[:max(n_kept, 1)])))   # (d_world is free between the chains)
        out["host_baseline"] = dict(method="cloudmetrics.planes (numpy)", files=nf, wall_ms_measured=host_s * 1e3, points_share=share, wall_ms_all_files_scaled=host_s * 1e3 / share,
                                    points_of_those_files=int(out_off[nf]), labels_differ=differs, upload_of_the_kept_points=up)
    return out


forms = {}
if HAS:
    for p in range(1, args.planes + 1):
        forms[f"planes_h{args.hyp}_r{p}"] = measure(out_off, args.hyp, p, host=p == args.planes)
    for h in [int(v) for v in args.hyp_list.split(",")]:
        if h != args.hyp:
            forms[f"planes_h{h}_r{args.planes}"] = measure(out_off, h, args.planes)
    if args.one_cloud:
        forms[f"one_cloud_h{args.hyp}_r{args.planes}"] = measure(np.array([0, n_map], dtype=np.uint64), args.hyp, args.planes)
after = chain()

print(f"{R} runs x {K} config-1 scans, {n_pts} registered points -> {F} map clouds of {n_map} points (leaf {args.leaf})")
for name, v in forms.items():
    print(f"  {name:22s}: {v['event_ms']['median']:8.3f} ms between events ({v['event_ms']['min']:.3f} .. {v['event_ms']['max']:.3f}), wall {v['wall_ms']['median']:.3f}; "
          + ", ".join(f"{n.replace('planes_', '')} {v[n + '_launch_ms']['median']:.3f}" for n in OWN)
          + f" ms; {v['score_tests']:.3e} tests, the score kernel at {v['score_fraction_of_nonfused_fp64_rate']:.3f} of the non-fused fp64 rate; planes {v['planes']} "
          f"({v['planes_per_round']} per round), on planes {v['on_planes']}, rest {v['rest']}, mean rmse {v['mean_rmse']}")
    if v.get("host_baseline"):
        hb = v["host_baseline"]
        print(f"    baseline: d2h {baseline['d2h']['wall_ms']['median']:.3f} ms + {hb['method']} {hb['wall_ms_measured']:.0f} ms for {nf} files, "
              f"{hb['wall_ms_all_files_scaled']:.0f} ms scaled to all files + upload {hb['upload_of_the_kept_points']['wall_ms']['median']:.3f} ms; labels that differ {hb['labels_differ']}")
for key in before:
    print(f"  {key:34s}: before {before[key]['event_ms']['median']:.3f} ms ({before[key]['event_ms']['min']:.3f} .. {before[key]['event_ms']['max']:.3f}), "
          f"after {after[key]['event_ms']['median']:.3f} ms ({after[key]['event_ms']['min']:.3f} .. {after[key]['event_ms']['max']:.3f})")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/map_planes.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, leaf=args.leaf,
                       reps=args.reps, warmup=args.warmup, registered_points=n_pts, map_clouds=F, map_points=n_map, seed=args.seed, forms=forms, baseline=baseline,
                       chain_before=before, chain_after=after), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_world, d_out, d_ref, d_kept, d_label, d_src)
