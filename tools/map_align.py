#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what aligning map clouds to a reference cloud costs (lk_clouds_align_dev), on
tools/map_c2c.py's workload - R runs of K consecutive config-1 scans replayed on the frozen map with d_world_out, cut into one file per run and
downsampled (lk_downsample_clouds_dev); the survey is the union of the first --ref-files map clouds downsampled once more.  Every pair (f, 0) starts
from a T0 that is a KNOWN perturbation of the identity (the map clouds lie in the survey's frame): --t0-deg degrees about a seeded axis through the
survey's centroid and --t0-m metres along a seeded direction; the JSON records them, the iterations taken as a distribution over the pairs, and how
far the final T lies from the identity.
ms: median over --reps timed calls after --warmup untimed ones, with min .. max, between two HIP events on the handle's stream - the whole call; one
search launch (a call with max_iter 0, profiling mode) and one solve launch (max_iter 1); the launch totals of the whole call.
Beside it, on the same clouds:
  route (a), what the parent commit offers per iteration: lk_clouds_c2c_dev with nn outputs on the moved clouds, lk_memcpy_d2h of the nn arrays and
             the clouds, a numpy Horn solve per file (over the first --host-files files, scaled by points), the moved clouds back up;
  route (b): lk_memcpy_d2h once, then an ICP with scipy.spatial.cKDTree on the host (first --host-files files, scaled by points), where scipy imports.
The accuracy form of lk_clouds_c2c_dev, the run replay and lk_downsample_clouds_dev are timed before and after (tools/map_c2c.py's figures).
--plane: the point-to-plane entry instead (lk_clouds_align_plane_dev) with the survey's normals from lk_clouds_normals_dev (--normal-radius,
--normal-min-pts, --normal-min-planarity), beside lk_clouds_align_dev on the same clouds and T0 in the same session; the normals entry is timed on the
survey and on the map clouds beside lk_clouds_mme_dev at the same radius; routes (a) and (b) are left out.
Usage: map_align.py [--plane] [--runs R] [--scans K] [--distinct D] [--leaf M] [--max-dist M] [--max-iter N] [--eps-rot RAD] [--eps-trans M] [--t0-deg DEG] [--t0-m M]
                    [--ref-files F] [--reps N] [--warmup W] [--host-files F] [--commit TEXT] [--json PATH]"""
import json
import os
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding, both, stats
from legkilo_amd import abi, cloudmetrics  # noqa: E402

try:
    from scipy.spatial import cKDTree
except ImportError:
    cKDTree = None

ap = rw.parser()
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--max-dist", type=float, default=0.25)
ap.add_argument("--max-iter", type=int, default=30)
ap.add_argument("--eps-rot", type=float, default=1e-5)
ap.add_argument("--eps-trans", type=float, default=1e-5)
ap.add_argument("--t0-deg", type=float, default=2.0)
ap.add_argument("--t0-m", type=float, default=0.1)
ap.add_argument("--ref-files", type=int, default=8)
ap.add_argument("--host-files", type=int, default=16)
ap.add_argument("--plane", action="store_true")
ap.add_argument("--normal-radius", type=float, default=0.3)
ap.add_argument("--normal-min-pts", type=int, default=5)
ap.add_argument("--normal-min-planarity", type=float, default=0.3)
args = ap.parse_args()

w = rw.Workload(args)
R, K, D, g, d_pts, d_imu, n_pts, x_run, P_run = w.R, w.K, w.D, w.g, w.d_pts, w.d_imu, w.n_pts, w.x, w.P
run_off, scan_off, tb, n_msg = w.run_off, w.scan_off, w.tb, w.n_msg
d_world, d_out, d_ref, d_moved = (g.device_malloc(16 * n_pts) for _ in range(4))
file_off, _ = binding.pcd_file_offsets(run_off, scan_off, K)
F = len(file_off) - 1
timer = rw.EventTimer(g, args)
timed = timer.timed
last = {}
md, thr = args.max_dist, (args.max_dist / 4, args.max_dist / 2, args.max_dist)


def replay():
    g.batch_replay_runs_cloud_dev(d_pts, run_off, scan_off, tb, 1, n_msg, d_imu, want_poses=False, d_world=d_world)


def downsample():
    last["out_off"], _ = g.downsample_clouds_dev(d_world, file_off, args.leaf, d_out)


def c2c():
    last["c2c"] = g.clouds_c2c_dev(d_out, out_off, d_ref, ref_off, pairs, md, thr)[0]


def chain():
    return dict(replay=both(timed(replay, before=lambda: g.batch_set_priors(x_run, P_run))), downsample=both(timed(downsample)), c2c_accuracy=both(timed(c2c)))


g.batch_set_priors(x_run, P_run)
replay()
downsample()
out_off = last["out_off"].copy()
n_map = int(out_off[-1])
ref_off, _ = g.downsample_clouds_dev(d_out, np.array([0, out_off[min(args.ref_files, F)]], dtype=np.uint64), args.leaf, d_ref)
n_ref = int(ref_off[-1])
pairs = [(f, 0) for f in range(F)]
before = chain()

# ---- the known perturbation: T0[f] = rotation by t0_deg about a seeded axis through the survey's centroid, then t0_m along a seeded direction
survey = np.zeros((n_ref, 4), dtype=np.float32)
g.d2h(survey, d_ref)
centre = survey[:, :3].astype(np.float64).mean(0)
rng = np.random.default_rng(1357)


def rodrigues(axis, angle):
    a = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


T0 = np.zeros((F, 12))
for f in range(F):
    Rm = rodrigues(rng.normal(size=3), np.deg2rad(args.t0_deg))
    d = rng.normal(size=3)
    T0[f] = np.r_[Rm.reshape(9), centre + args.t0_m * d / np.linalg.norm(d) - Rm @ centre]


def align(max_iter=args.max_iter, key="align"):
    def call():
        last[key] = g.clouds_align_dev(d_out, out_off, d_ref, ref_off, pairs, md, T0, max_iter, args.eps_rot, args.eps_trans, thr)
    return call


def align_plane(max_iter=args.max_iter, key="plane"):
    def call():
        last[key] = g.clouds_align_plane_dev(d_out, out_off, d_ref, ref_off, d_nrm, pairs, md, T0, max_iter, args.eps_rot, args.eps_trans, thr)
    return call


def measure(make, key, solve):
    """One alignment entry on the workload: the whole call, its launch totals and counts, one search launch, one solve launch, what the pairs did."""
    whole = timed(make())
    rec, crec = last[key][0], last[key][-2]
    launches = ("align_init", "align_search", solve, "c2c_reduce")
    tot = rw.per_launch(g, make(), launches, args.reps)
    counts = {}
    g.profile_reset(), g.profile_enable(True)
    make()()
    for k in launches:
        counts[k] = int(g.profile_get(k)[0])
    g.profile_enable(False)
    one_search = rw.per_launch(g, make(0, key + "0"), ("align_search",), args.reps, count=1)["align_search"]
    one_solve = rw.per_launch(g, make(1, key + "1"), ("align_search", solve), args.reps)[solve]
    extra = {}
    if solve == "align_plane_solve":            # (with max_iter 1 the kernel runs twice: the solve, then the closing first pass, which max_iter 0 runs alone)
        closing = rw.per_launch(g, make(0, key + "0"), (solve,), args.reps, count=1)[solve]
        one_solve = [max(v - float(np.median(closing)), 0.0) for v in one_solve]
        extra["one_closing_pass_launch_ms"] = stats(closing)
    angle = np.degrees(np.arccos(np.clip((rec["rot"][:, 0] + rec["rot"][:, 4] + rec["rot"][:, 8] - 1) / 2, -1, 1)))
    shift = np.linalg.norm(rec["rot"].reshape(-1, 3, 3) @ centre + rec["trans"] - centre, axis=1)
    iters = rec["iters"].astype(int)
    return dict(max_dist=md, max_iter=args.max_iter, eps_rot=args.eps_rot, eps_trans=args.eps_trans, pairs=F, query_points=int(crec["n_query"].sum()), reference_points=n_ref,
                t0=dict(degrees=args.t0_deg, metres=args.t0_m, about="the survey's centroid", seed=1357), **both(whole),
                one_search_launch_ms=stats(one_search), one_solve_launch_ms=stats(one_solve), **extra, launches_per_call=counts,
                launch_totals_ms={k: stats(v) for k, v in tot.items()},
                iterations=dict(histogram={str(k): int((iters == k).sum()) for k in sorted(set(iters.tolist()))}, mean=float(iters.mean()), max=int(iters.max())),
                converged_pairs=int(((rec["status"] & abi.LK_ALIGN_CONVERGED) != 0).sum()), few_pairs=int(((rec["status"] & abi.LK_ALIGN_FEW) != 0).sum()),
                degenerate_pairs=int(((rec["status"] & abi.LK_ALIGN_DEGENERATE) != 0).sum()),
                bad_pairs=int((rec["status"] & 19 != 0).sum()), rmse_first_median=float(np.nanmedian(rec["rmse_first"])), rmse_last_median=float(np.nanmedian(crec["rmse"])),
                matched_first=int(rec["n_matched_first"].sum()), matched_last=int(crec["n_matched"].sum()),
                final_T_from_identity=dict(degrees_median=float(np.median(angle)), degrees_max=float(angle.max()), metres_at_centroid_median=float(np.median(shift)),
                                           metres_at_centroid_max=float(shift.max())))


def show(name, form):
    print(f"  {name}: {form['event_ms']['median']:.3f} ms between events ({form['event_ms']['min']:.3f} .. {form['event_ms']['max']:.3f}), wall {form['wall_ms']['median']:.3f}; "
          f"one search {form['one_search_launch_ms']['median']:.3f} ms, one solve {form['one_solve_launch_ms']['median']:.3f} ms; launches {form['launches_per_call']}")
    print("  launch totals: " + ", ".join(f"{k} {v['median']:.3f}" for k, v in form["launch_totals_ms"].items()))
    print(f"  iterations {form['iterations']}, converged {form['converged_pairs']}, degenerate {form['degenerate_pairs']}, few {form['few_pairs']}, bad {form['bad_pairs']}; "
          f"rmse {form['rmse_first_median']:.4f} -> {form['rmse_last_median']:.4f} m; final T from the identity: {form['final_T_from_identity']}")


def chain_lines():
    for k in ("replay", "downsample", "c2c_accuracy"):
        print(f"  {k:12s}: before {before[k]['event_ms']['median']:.3f} ms ({before[k]['event_ms']['min']:.3f} .. {before[k]['event_ms']['max']:.3f}), "
              f"after {after[k]['event_ms']['median']:.3f} ms ({after[k]['event_ms']['min']:.3f} .. {after[k]['event_ms']['max']:.3f})")


if args.plane:
    d_nrm, d_map_nrm = g.device_malloc(16 * max(n_ref, 1)), g.device_malloc(16 * n_map)
    nr_args = (args.normal_radius, args.normal_min_pts, args.normal_min_planarity)

    def normals_survey():
        last["nrm"] = g.clouds_normals_dev(d_ref, ref_off, nr_args[0], d_nrm, nr_args[1], nr_args[2])

    def normals_map():
        last["nrm_map"] = g.clouds_normals_dev(d_out, out_off, nr_args[0], d_map_nrm, nr_args[1], nr_args[2])

    def mme_survey():
        g.clouds_mme_dev(d_ref, ref_off, nr_args[0], max(nr_args[1], 4))

    def mme_map():
        g.clouds_mme_dev(d_out, out_off, nr_args[0], max(nr_args[1], 4))

    normals = dict(radius=nr_args[0], min_pts=nr_args[1], min_planarity=nr_args[2], survey=both(timed(normals_survey)), survey_mme_same_radius=both(timed(mme_survey)),
                   map_clouds=both(timed(normals_map)), map_clouds_mme_same_radius=both(timed(mme_map)))
    normals.update(survey_valid=int(last["nrm"]["n_valid"].sum()), survey_points=n_ref, map_valid=int(last["nrm_map"]["n_valid"].sum()), map_points=n_map)
    normals_survey()
    plane = measure(align_plane, "plane", "align_plane_solve")
    pl = last["plane"][1]
    plane.update(used_first=int(pl["n_used_first"].sum()), used_last=int(pl["n_used"].sum()), rmse_plane_first_median=float(np.nanmedian(pl["rmse_plane_first"])),
                 rmse_plane_last_median=float(np.nanmedian(pl["rmse_plane"])))
    point = measure(align, "align", "align_solve")
    after = chain()
    print(f"{R} runs x {K} config-1 scans -> {F} map clouds of {n_map} points (leaf {args.leaf}), survey of {n_ref} points; T0 {args.t0_deg} deg, {args.t0_m} m")
    print(f"  normals (radius {nr_args[0]}, min_pts {nr_args[1]}, planarity {nr_args[2]}): survey {normals['survey']['event_ms']['median']:.3f} ms "
          f"({normals['survey_valid']} of {n_ref} valid; mme {normals['survey_mme_same_radius']['event_ms']['median']:.3f} ms), map clouds "
          f"{normals['map_clouds']['event_ms']['median']:.3f} ms ({normals['map_valid']} of {n_map} valid; mme {normals['map_clouds_mme_same_radius']['event_ms']['median']:.3f} ms)")
    show("point-to-plane", plane)
    print(f"  used {plane['used_first']} -> {plane['used_last']}, plane rmse {plane['rmse_plane_first_median']:.4f} -> {plane['rmse_plane_last_median']:.5f} m")
    show("point-to-point", point)
    chain_lines()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/map_align.py --plane", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D,
                           leaf=args.leaf, reps=args.reps, warmup=args.warmup, registered_points=n_pts, map_clouds=F, map_points=n_map, survey_points=n_ref,
                           ref_files=args.ref_files, normals=normals, align_plane=plane, align=point, chain_before=before, chain_after=after), f, indent=1)
            f.write("\n")
    timer.close()
    w.close(d_world, d_out, d_ref, d_moved, d_nrm, d_map_nrm)
    raise SystemExit(0)

form = measure(align, "align", "align_solve")
counts = form["launches_per_call"]
iters = last["align"][0]["iters"].astype(int)

# ---- route (a): one iteration the parent commit's way - C2C with nn outputs on the moved clouds, everything down, a numpy Horn solve per file, the clouds up
g.clouds_transform_dev(d_out, out_off, T0, d_moved)
total = n_map
d_idx, d_d2 = g.device_malloc(4 * total), g.device_malloc(8 * total)
maps, moved = np.zeros((n_map, 4), dtype=np.float32), np.zeros((n_map, 4), dtype=np.float32)
idx, d2 = np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.float64)
nf = min(args.host_files, F)
share = float(out_off[nf]) / n_map
s64 = survey[:, :3].astype(np.float64)


def c2c_nn():
    g.clouds_c2c_dev(d_moved, out_off, d_ref, ref_off, pairs, md, thr, d_idx, d_d2)


def down():
    g.d2h(idx, d_idx), g.d2h(d2, d_d2), g.d2h(moved, d_moved)


def up():
    g.h2d(d_moved, moved)


def horn_files():
    for f in range(nf):
        lo, hi = int(out_off[f]), int(out_off[f + 1])
        m = idx[lo:hi] != cloudmetrics.NO_MATCH
        P, G = moved[lo:hi, :3][m].astype(np.float64), s64[idx[lo:hi][m]]
        pbar, rbar = P.mean(0), G.mean(0)
        Rn = cloudmetrics.horn_rotation((P - pbar).T @ (G - rbar))
        moved[lo:hi, :3] = (moved[lo:hi, :3].astype(np.float64) @ Rn.T + (rbar - Rn @ pbar)).astype(np.float32)


ra = dict(c2c_with_nn=both(timed(c2c_nn)), d2h=dict(bytes=int(idx.nbytes + d2.nbytes + moved.nbytes), **both(timed(down))))
t1 = time.perf_counter()
horn_files()
solve_s = time.perf_counter() - t1
ra["numpy_solve"] = dict(files=nf, wall_ms_measured=solve_s * 1e3, points_share=share, wall_ms_all_files_scaled=solve_s * 1e3 / share)
ra["h2d"] = dict(bytes=int(moved.nbytes), **both(timed(up)))
ra["per_iteration_ms"] = ra["c2c_with_nn"]["event_ms"]["median"] + ra["d2h"]["wall_ms"]["median"] + ra["numpy_solve"]["wall_ms_all_files_scaled"] + ra["h2d"]["wall_ms"]["median"]
ra["for_the_mean_iterations_ms"] = ra["per_iteration_ms"] * form["iterations"]["mean"]


# ---- route (b): the clouds down once, an ICP with a k-d tree on the host
def fetch():
    g.d2h(maps, d_out), g.d2h(survey, d_ref)


rb = dict(d2h=dict(bytes=int(maps.nbytes + survey.nbytes), **both(timed(fetch))))
if cKDTree is not None:
    t1 = time.perf_counter()
    tree = cKDTree(s64)
    host_iters = []
    for f in range(nf):
        q = maps[int(out_off[f]):int(out_off[f + 1]), :3].astype(np.float64)
        T = T0[f].copy()
        for it in range(args.max_iter):
            mv = q @ T[:9].reshape(3, 3).T + T[9:]
            dist, j = tree.query(mv, distance_upper_bound=md)
            m = np.isfinite(dist)
            if m.sum() < 3:
                break
            pbar, rbar = q[m].mean(0), s64[j[m]].mean(0)
            Rn = cloudmetrics.horn_rotation((q[m] - pbar).T @ (s64[j[m]] - rbar))
            Tn = np.r_[Rn.reshape(9), rbar - Rn @ pbar]
            sr, st = cloudmetrics.align_step(T, Tn, pbar)
            T = Tn
            if sr <= args.eps_rot and st <= args.eps_trans:
                break
        host_iters.append(it + 1)
    host_s = time.perf_counter() - t1
    rb["host"] = dict(method="scipy.spatial.cKDTree, one tree on the survey", files=nf, wall_ms_measured=host_s * 1e3, points_share=share,
                      wall_ms_all_files_scaled=host_s * 1e3 / share, iterations_mean=float(np.mean(host_iters)),
                      device_iterations_mean_same_files=float(iters[:nf].mean()))
else:
    rb["host"] = dict(method="not measured: scipy does not import")
after = chain()

print(f"{R} runs x {K} config-1 scans -> {F} map clouds of {n_map} points (leaf {args.leaf}), survey of {n_ref} points; T0 {args.t0_deg} deg, {args.t0_m} m")
show("align", form)
print(f"  route (a) per iteration: c2c+nn {ra['c2c_with_nn']['event_ms']['median']:.2f} + d2h {ra['d2h']['wall_ms']['median']:.2f} + numpy solve "
      f"{ra['numpy_solve']['wall_ms_all_files_scaled']:.0f} + h2d {ra['h2d']['wall_ms']['median']:.2f} = {ra['per_iteration_ms']:.0f} ms; x {form['iterations']['mean']:.2f} iterations = "
      f"{ra['for_the_mean_iterations_ms']:.0f} ms")
print(f"  route (b): d2h {rb['d2h']['wall_ms']['median']:.2f} ms + {rb['host']}")
chain_lines()
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/map_align.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D, leaf=args.leaf,
                       reps=args.reps, warmup=args.warmup, registered_points=n_pts, map_clouds=F, map_points=n_map, survey_points=n_ref, ref_files=args.ref_files,
                       align=form, route_a=ra, route_b=rb, chain_before=before, chain_after=after), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_world, d_out, d_ref, d_moved, d_idx, d_d2)
