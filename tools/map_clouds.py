#!/usr/bin/env python
"""Measurement on one MI355X, everything through the C-ABI: what the downsampled map clouds cost (lk_downsample_clouds_dev), on the workload of
tools/runs_workload.py - R runs of K consecutive config-1 scans replayed on the frozen map with d_world_out (lk_batch_replay_runs_cloud_dev), which
is the input here and stays in HBM.  Forms:
  files_<n>   pcd_file_offsets(..., frames_per_file = n) for every n of --frames-per-file: R * ceil(K / n) files in one call, leaf --leaf;
  one_file    the same points as ONE file (the skewed shape: a single file takes the device-wide sort instead of a segment per file);
  d2h         what the parent commit offers, first half: lk_memcpy_d2h of the whole registered cloud;
  numpy       ... second half: the numpy restatement (oracle/preprocess_oracle.py::voxel_grid_centroid) file by file on the host copy, over the first
              --numpy-files files of the first files_<n> form, wall clock, scaled to all files by the point counts.  The device's records of those
              files must be the restatement's bits.
ms per call: median over --reps timed calls after --warmup untimed ones, with min .. max, twice: between two HIP events on the handle's stream
(the call is synchronous, the events bracket it) and by the host's wall clock.  Bandwidth: the chain's own byte count of DESIGN.md section 4i,
132 B per point + 24 B per cell, over the event time.
Usage: map_clouds.py [--runs R] [--scans K] [--distinct D] [--frames-per-file LIST] [--leaf M] [--reps N] [--warmup W] [--numpy-files F] [--commit TEXT] [--json PATH]"""
import json
import os
import sys
import time

import numpy as np

import runs_workload as rw
from runs_workload import binding, stats

sys.path.insert(0, os.path.join(rw.ROOT, "oracle"))   # preprocess_oracle.py: the numpy definition the baseline runs (measurement only)
import preprocess_oracle as po  # noqa: E402

BYTES_PER_POINT, BYTES_PER_CELL = 132, 24
COPY_CEILING_TBS = 6.29                     # the measured device-to-device copy rate of this card

ap = rw.parser()
ap.add_argument("--frames-per-file", default="4,2")
ap.add_argument("--leaf", type=float, default=0.1)
ap.add_argument("--numpy-files", type=int, default=32, help="files of the host baseline (it costs ~10 ms per file)")
args = ap.parse_args()

w = rw.Workload(args)
R, K, D, g, d_pts, d_imu, n_pts, run_off, scan_off, tb, n_msg = w.R, w.K, w.D, w.g, w.d_pts, w.d_imu, w.n_pts, w.run_off, w.scan_off, w.tb, w.n_msg
d_world, d_out = g.device_malloc(16 * n_pts), g.device_malloc(16 * n_pts)
g.batch_set_priors(w.x, w.P)
g.batch_replay_runs_cloud_dev(d_pts, run_off, scan_off, tb, 1, n_msg, d_imu, want_poses=False, d_world=d_world)   # the input: the registered cloud

timer = rw.EventTimer(g, args)
timed = timer.timed
forms, last = {}, {}


def device_form(name, file_off):
    def call():
        last["out_off"], last["unf"] = g.downsample_clouds_dev(d_world, file_off, args.leaf, d_out)

    res = timed(call)
    cells = int(last["out_off"][-1])
    sizes = np.diff(file_off.astype(np.int64))
    e = stats([a for a, _ in res])
    nbytes = BYTES_PER_POINT * n_pts + BYTES_PER_CELL * cells
    forms[name] = dict(files=len(file_off) - 1, points=n_pts, largest_file=int(sizes.max()), smallest_file=int(sizes.min()), cells=cells,
                       unfiltered_files=int(last["unf"].sum()), event_ms=e, wall_ms=stats([b for _, b in res]), chain_bytes=nbytes,
                       tb_per_s=nbytes / (e["median"] * 1e-3) / 1e12, ns_per_point=e["median"] * 1e6 / n_pts)
    return last["out_off"].copy()


fpfs = [int(v) for v in args.frames_per_file.split(",")]
first = None
for n in fpfs:
    fo, _ = binding.pcd_file_offsets(run_off, scan_off, n)
    oo = device_form(f"files_{n}", fo)
    if first is None:
        out = np.zeros((int(oo[-1]), 4), dtype=np.float32)
        g.d2h(out, d_out)
        first = (n, fo, oo, out)
device_form("one_file", np.array([0, n_pts], dtype=np.uint64))

# the parent commit's route: the cloud to the host, the numpy restatement file by file
cloud = np.zeros((n_pts, 4), dtype=np.float32)
res = timed(lambda: g.d2h(cloud, d_world))
forms["d2h"] = dict(bytes=16 * n_pts, event_ms=stats([a for a, _ in res]), wall_ms=stats([b for _, b in res]), what="lk_memcpy_d2h of the registered cloud (parent commit's route, first half)")
n0, fo, oo, out = first
nf = min(args.numpy_files, len(fo) - 1)
t1 = time.perf_counter()
for f in range(nf):
    want = po.voxel_grid_centroid(cloud[int(fo[f]):int(fo[f + 1])].view(po.OUT_DTYPE).reshape(-1), args.leaf)
    got = out[int(oo[f]):int(oo[f + 1])]
    assert np.array_equal(np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4), got.view(np.uint32)), f"file {f}: the device's records are not the restatement's"
host_s = time.perf_counter() - t1
share = float(fo[nf] - fo[0]) / n_pts
forms["numpy"] = dict(files=nf, of_form=f"files_{n0}", wall_ms_measured=host_s * 1e3, points_share=share, wall_ms_all_files_scaled=host_s * 1e3 / share,
                      bit_equal_files=nf, what="numpy restatement per file on the host copy (parent commit's route, second half): one pass, wall clock, scaled by points")

pps = n_pts / (R * K)
print(f"{R} runs x {K} config-1 scans ({pps:.0f} points per scan, {n_pts} points), leaf {args.leaf}, {args.reps} timed calls after {args.warmup} warm-up calls")
for name, v in forms.items():
    if "cells" in v:
        print(f"  {name:9s}: {v['event_ms']['median']:9.3f} ms between events ({v['event_ms']['min']:.3f} .. {v['event_ms']['max']:.3f}), wall {v['wall_ms']['median']:.3f} ms; "
              f"{v['files']} files (largest {v['largest_file']}), {v['cells']} cells, {v['unfiltered_files']} unfiltered; {v['tb_per_s']:.3f} TB/s of {BYTES_PER_POINT} B/point + {BYTES_PER_CELL} B/cell")
print(f"  d2h      : {forms['d2h']['wall_ms']['median']:9.3f} ms wall ({forms['d2h']['wall_ms']['min']:.3f} .. {forms['d2h']['wall_ms']['max']:.3f}) for {16 * n_pts} bytes")
print(f"  numpy    : {forms['numpy']['wall_ms_measured']:9.1f} ms wall for {nf} files of files_{n0} (bit-equal to the device), {forms['numpy']['wall_ms_all_files_scaled']:.0f} ms scaled to all files")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/map_clouds.py", commit=args.commit, library=os.path.basename(binding.LIB_PATH), runs=R, scans_per_run=K, distinct_segments=D,
                       leaf=args.leaf, reps=args.reps, warmup=args.warmup, map_scans=args.map_scans, points_per_scan=pps, bytes_per_point=BYTES_PER_POINT,
                       bytes_per_cell=BYTES_PER_CELL, copy_ceiling_tb_per_s=COPY_CEILING_TBS, forms=forms), f, indent=1)
        f.write("\n")
timer.close()
w.close(d_world, d_out)
