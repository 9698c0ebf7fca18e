#!/usr/bin/env python
"""bench.py — LiDAR scans/s through the per-time-bucket ESKF update on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N>1: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W; without a launcher
     `python bench.py --gpus N` starts its N ranks itself, the same way)

Workload (BASELINE.json metric "LiDAR scans/sec (per-point ESKF update), 100k-pt scan, 1->8 MI355X"), config 5 with
config 3's per-scan semantics:
  one step = one batch of `--scans-per-gpu` (1024) synthetic 100 000-point scans per GPU, EVERY scan distinct (scan g:
  ray seed 5005+g, its own pose on the trajectory, its own prior = pose (+) N(0, 2 cm / 0.5 deg)), each run through the
  full per-bucket ESKF update (5 time buckets x 20 000 points: predict -> voxel-hash plane matching + residual rows +
  A/b reduction -> 6x6 information-form update) against ONE shared voxel map, frozen (inserts disabled on GPU and
  oracle alike).  Scans and priors are resident in HBM before the timed region.  Inside a time bucket the points come
  in the order the reference's pipeline hands them over: pcl::VoxelGrid's output order (KILO.cc:356-370).
  N>1: rank 0 builds the map and broadcasts the device blob over RCCL; scans are sharded with no data-path collective;
  per-step poses are all-gathered.  Default = weak scaling (1024 scans per GPU); `--total-scans 1024` = strong scaling
  (BASELINE config 5 as worded: 1024 scans in total, 128 per GPU at N = 8); the JSON line says which.
With --full the line is self-checking: the cpu_baseline leg replays a sample of the batch through the oracle ON THE MAP THE DEVICE
HOLDS and compares counts and poses with what the TIMED loop delivered for the same scans (`parity_check`; a violation
exits non-zero).  `roofline` describes lk_residual_kernel with counter-derived bounds (profiles/latest_pmc.json, made
by tools/gpu_prof_r02.sh + tools/collect_r02.py from rocprofv3 --pmc passes of this very command): HBM fraction from FETCH_SIZE/WRITE_SIZE,
L2 fraction from TCC_REQ, VALU-issue fraction from SQ_INSTS_VALU, launch time from the timed region.
`cpu_baseline` = the oracle (kind "port") on one pinned host thread, plus the reference's own build (oracle/_ref,
literal N x N update) timed on the config-1 scans for the record.

A plain run does only what the headline needs: it generates the batch and the map's scans, builds the map, uploads and prepares
the batch, runs the W warm-up and K timed steps, writes --dump-outputs and prints the line (`value`, `ms_per_step`, `roofline` from
the timed region and the stored counters; `cpu_baseline` and `parity_check` null).  Everything else it measures or checks - the
parity check and CPU baselines, the sustained / shard128 / shuffled-order / PCIe / overlay / config-1, -2, -3, -4 extras, the
kernel-event pass, the second map transport at N > 1 - runs with `--full`.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

T_PROCESS0 = time.time()   # extra.setup_s: what a run spends before its first warm-up step, from here
ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lk_pkg  # noqa: E402

lk_pkg.load()
from legkilo_amd import abi as _abi  # noqa: E402
from legkilo_amd import binding, config, replay, synth  # noqa: E402

ALG_BYTES_SURVEY = 288     # scan pt 16 + hash slot 16 + plane record 240 + world pt 16
ALG_BYTES_RESIDUAL = 176   # what THIS layout touches per point in batch replay: scan pt 16 + hash slot 16 + 144-B match record
ALG_BYTES_FULL = 1016      # + update pass 728 (re-projection write, map append, amortised refit)
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_COPY_CEILING_GBS = 6290.0
L2_PEAK_GBS = 34500.0      # same guide: aggregate L2 bandwidth
SIMDS, CLK_GHZ = 1024, 2.4
N_PTS = 100_000
N_BUCKETS = 5
PMC_FILE = os.path.join(ROOT, "profiles", "latest_pmc.json")
FP64_PEAK_TFLOPS = 78.6    # AMD MI355X datasheet: peak fp64 vector = fp64 matrix = 78.6 TFLOP/s (MI355X_MICROARCH.md has no fp64 row; 256 CUs x 4 SIMDs x 16 fp64 FMA lanes x 2 flop x 2.4 GHz = 78.6)
COMPULSORY_BYTES_PER_POINT = 20   # what HBM must carry per point of the batch residual pass: 16 B scan point + 4 B of its tile's partial record
OV_PMC_FILE = os.path.join(ROOT, "profiles", "latest_overlay_pmc.json")
C2_PMC_FILE = os.path.join(ROOT, "profiles", "latest_config2_pmc.json")
C2_BYTES_PER_POINT = 81    # config 2 with the rows materialised: 16 B scan point in + h6 48 + z 8 + R 8 + valid 1 out ("+64 B/pt if h/z/R rows are materialised")
OV_KERNELS = ("ov_reset", "predict", "ov_residual", "update", "ov_begin", "ov_reproject", "ov_materialise", "ov_point_geom", "ov_root_lane", "ov_insert_root", "ov_fit_eig", "ov_fit_lane",
              "ov_insert_apply", "ov_insert_fallback")
OV_KERNEL_SOURCES = ("lk_overlay_kernels.h", "lk_map_kernels.h", "lk_device.h")
# config 4's sensor message: the fields of an Ouster PointCloud2 point that LidarProcessing::ousterHander reads (lidar_processing.cc:54-80)
OUSTER_MSG_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<u4")])
OUSTER_MSG_LAYOUT = dict(point_step=16, off_x=0, off_y=4, off_z=8, off_time=12, lidar_type=2)
T0_CONFIG4 = 3.0
RAGOV_PMC_FILE = os.path.join(ROOT, "profiles", "latest_ragged_overlay_pmc.json")
RAGOV_KERNEL_SOURCES = ("lk_ovscan.hip", "lk_overlay_kernels.h", "lk_map_kernels.h", "lk_filter_kernels.h", "lk_point_kernels.h", "lk_device.h")   # what the scan-resident overlay kernel is made of
KERNEL_SOURCES = ("lk_point_kernels.h", "lk_device.h")   # where the batch residual kernel lives (lk_residual_kernel, residual_tile, geometry)


def kernel_sources_sha16(files=KERNEL_SOURCES):
    """Fingerprint of the batch residual kernel's sources: tools/collect_r03.py stores it beside the counters it collects, and the
    bench line warns when the kernel has changed since (the counters then describe an older kernel)."""
    import hashlib

    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(ROOT, "leg-kilo_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def overlay_roofline(kernel_ms, launches, n_scans, warnings):
    """Counter-derived roofline object of the batch WITH insert (extra.overlay_roofline).  profiles/latest_overlay_pmc.json (tools/collect_overlay_pmc.py,
    from separate `rocprofv3 --pmc` passes of tools/overlay_prof.py) holds, per lk_ov_* kernel and launch: HBM bytes (2 x FETCH_SIZE + WRITE_SIZE, the guide's
    gfx950 correction), VALU instructions, waves, VGPRs / scratch / waves per SIMD.  The launch durations are THIS run's (HIP events, one stream).  The dominant
    kernel is the one with the most time in this run."""
    out = {"bound": "hbm+latency", "peak": HBM_PEAK_GBS, "unit": "GB/s"}
    if not os.path.exists(OV_PMC_FILE):
        out["pmc_source"] = None
        warnings.append("profiles/latest_overlay_pmc.json missing: extra.overlay_roofline has durations only (tools/gpu_prof_overlay.sh)")
        pmc = {}
    else:
        pmc = json.load(open(OV_PMC_FILE))
        out["pmc_source"] = f"profiles/latest_overlay_pmc.json (tag {pmc.get('tag')}, commit {pmc.get('commit')}, {pmc.get('slots')} slots)"
        if pmc.get("kernel_sources_sha16") != kernel_sources_sha16(OV_KERNEL_SOURCES):
            warnings.append(f"overlay counters (profiles/latest_overlay_pmc.json, tag {pmc.get('tag')}) were collected on a different version of "
                            f"{', '.join(OV_KERNEL_SOURCES)}: re-run tools/gpu_prof_overlay.sh")
    per = {}
    tot_bytes, tot_ms = 0.0, 0.0
    for k, ms in kernel_ms.items():
        if not k.startswith("ov_") or not launches.get(k):
            continue
        c = (pmc.get("kernels") or {}).get(k)
        e = {"ms_per_batch": ms, "launches": launches[k], "ms_per_launch": round(ms / launches[k], 4)}
        if c:
            scale = n_scans / float(pmc.get("slots") or n_scans)   # counters are per REPLAY of the profiled batch (its launches differ: three slot groups there)
            gb = c["hbm_bytes_per_replay"] * scale / launches[k] / 1e9
            e.update({"hbm_GB_per_launch": round(gb, 3), "achieved_GBs": round(gb / (ms / launches[k] * 1e-3), 1),
                      "frac": round(gb / (ms / launches[k] * 1e-3) / HBM_PEAK_GBS, 4),
                      "valu_issue_frac": None if not c.get("valu_insts_per_replay") else round(c["valu_insts_per_replay"] * scale * 4.0 / (SIMDS * CLK_GHZ * 1e9 * ms * 1e-3), 3),
                      "vgprs": c.get("vgprs"), "scratch_bytes": c.get("scratch"), "waves_per_simd": c.get("waves_per_simd")})
            tot_bytes += gb * launches[k]
            tot_ms += ms
        per[k] = e
    if per:
        dom = max(per, key=lambda k: per[k]["ms_per_batch"])
        out["kernel"] = "lk_" + dom + "_kernel"
        out.update({k: v for k, v in per[dom].items() if k in ("achieved_GBs", "frac", "hbm_GB_per_launch", "valu_issue_frac", "vgprs", "scratch_bytes", "waves_per_simd", "ms_per_launch")})
        out["achieved"] = per[dom].get("achieved_GBs")
        out["traffic"] = None if "hbm_GB_per_launch" not in per[dom] else round(per[dom]["hbm_GB_per_launch"] * 1e9)
    out["per_kernel"] = per
    if tot_ms > 0:
        out["all_overlay_kernels"] = {"hbm_GB_per_batch": round(tot_bytes, 2), "achieved_GBs_over_kernel_time": round(tot_bytes / (tot_ms * 1e-3), 1),
                                      "frac": round(tot_bytes / (tot_ms * 1e-3) / HBM_PEAK_GBS, 4)}
    return out


def pts_per_launch_of(S):
    return S * (N_PTS // N_BUCKETS)


class Frozen:
    def __init__(self, tr, t):
        self.tr, self.t = tr, t

    def rot(self, tt):
        return self.tr.rot(np.full(np.shape(tt), self.t))

    def pos(self, tt):
        return self.tr.pos(np.full(np.shape(tt), self.t))


def xyz_of(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float32)


def world_of(x36, xyz_body, P):
    R = x36[:9].reshape(3, 3)
    E = np.array(P["extrinsic_R"], float).reshape(3, 3)
    T = np.array(P["extrinsic_T"], float)
    return ((xyz_body.astype(np.float64) @ E.T + T) @ R.T + x36[9:12]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- synthetic inputs
# All generation runs in a fork pool BEFORE the process touches the GPU (1024 ray-cast scans are ~0.4 s each on one core).
_W = _T = None


def _init_worker():
    global _W, _T
    _W, _T = synth.World(), synth.Trajectory()
    try:
        os.sched_setaffinity(0, range(os.cpu_count()))
    except Exception:
        pass


def scan_time(t_after, g):
    """Start time of batch scan g: 1024 poses spread over 51.2 s of the 60 s figure-eight; later thousands interleave."""
    return t_after + 0.05 * (g % 1024) + 0.0137 * (g // 1024)


def _gen(job):
    kind, a = job
    P = config.LEG_FUSION
    if kind == "dense":
        tb, nb, s_scan, s_noise = a
        return synth.dense_scan(_W, _T, tb, P, n=N_PTS, n_buckets=nb, seed_scan=s_scan, seed_noise=s_noise)
    if kind == "first":
        (t0,) = a
        return synth.dense_scan(_W, Frozen(_T, t0), t0, P, n=N_PTS, n_buckets=1, seed_scan=777)
    if kind == "vlp":
        tb, s_noise = a
        raw = synth.vlp16_scan(_W, _T, tb, P, seed_noise=s_noise)
        pre = synth.preprocess_velodyne(raw, P["filter_num"], P["blind"])
        return synth.sort_by_time(synth.voxel_grid_centroid(pre, P["voxel_grid_resolution"]))
    if kind == "ouster":   # config 4: an OS1-64-like message of the diter configuration (x, y, z f32 + the point's `t` in ns)
        tb, s_noise, static = a
        pts, t_ns = synth.ouster_scan(_W, Frozen(_T, tb) if static else _T, tb, config.DITER, seed_noise=s_noise)
        raw = np.zeros(len(pts), dtype=OUSTER_MSG_DTYPE)
        raw["x"], raw["y"], raw["z"], raw["t"] = pts["x"], pts["y"], pts["z"], t_ns
        return raw
    raise ValueError(kind)


def generate(jobs, workers):
    if workers <= 1 or len(jobs) < 4:
        _init_worker()
        return [_gen(j) for j in jobs]
    import multiprocessing as mp

    with mp.get_context("fork").Pool(workers, initializer=_init_worker) as pool:
        return pool.map(_gen, jobs, chunksize=max(1, len(jobs) // (workers * 4)))


def build_map(obj, traj, P, first, warm, warm_t):
    """First frame (dense static cloud) + warm-up scans through the full path WITH inserts, each from the true pose of its
    start time (mapping with known poses): the shared snapshot covers the whole trajectory the batch's 1024 poses lie on."""
    t0 = warm_t[0]
    x0 = synth.initial_state(traj, t0, P)
    obj.set_state(x0, 1e-6 * np.eye(30))
    obj.init_process_cov_q()
    obj.set_acc_norm(9.81)
    obj.set_times(t0, t0)
    xb = xyz_of(first)
    obj.map_build(world_of(x0, xb, P), xb)
    for pts, tb in zip(warm, warm_t):
        obj.set_state(synth.initial_state(traj, tb, P), 1e-6 * np.eye(30))
        obj.set_times(tb, tb)
        obj.process_scan(pts, tb)


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, poses, x36, P900):
    """--dump-outputs: what the timed path handed its caller in the last timed step - per scan the pose record copied to the host (lk_pose)
    and the filter slot's state record (state 36 + covariance 900) - one float64 .npy per array, so that two builds can be compared output for
    output.  Beyond DUMP_MAX_BYTES a fixed, seeded sample of the scans is written (scan_index.npy names them)."""
    arrays = {"pose_rot": poses["rot"], "pose_pos": poses["pos"], "pose_vel": poses["vel"], "pose_n_effect": poses["n_effect"],
              "pose_n_buckets": poses["n_buckets"], "pose_n_updates": poses["n_updates"], "state_x36": x36, "state_P900": P900}
    n = len(poses)
    assert all(len(a) == n for a in arrays.values()), {k: len(a) for k, a in arrays.items()}
    row_bytes = 8 * (1 + sum(int(np.prod(a.shape[1:])) for a in arrays.values()))
    idx = np.arange(n)
    if n * row_bytes > DUMP_MAX_BYTES:
        idx = np.sort(np.random.default_rng(20260).choice(n, DUMP_MAX_BYTES // row_bytes, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "scan_index.npy"), idx.astype(np.float64))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(np.asarray(a)[idx], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 30 untimed + 40 timed steps (~0.12 s of GPU time).  A region this short is sensitive to where the clocks are when it
    # starts: after the idle set-up phase 3 warm-up steps (5 ms) leave ~1.7 ms of ramp inside a 20-step region (1.775 vs 1.69 ms per
    # step; `--step-sweep`: elapsed(K) = 0.15 + 1.685 K ms once warm); `extra.sustained_*` is the >= 1 s figure
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--ramp-steps", type=int, default=0, help="untimed steps BEFORE the warm-up steps (clocks up after the idle set-up phase): with --warmup 5 "
                    "~3 %% of ramp sits inside a 20-step region.  Default 0 = exactly the protocol the driver asks for (W warm-up steps, K timed steps), as in "
                    "rounds 1-3; round 4's line had 30 (disclosed); `extra.sustained_*` is the clocks-up figure")
    ap.add_argument("--scans-per-gpu", type=int, default=1024, help="weak scaling: a batch of 1024 scans per GPU (fits one GPU)")
    ap.add_argument("--total-scans", type=int, default=0, help="strong scaling: this many scans in total, block-sharded over the GPUs "
                    "(BASELINE config 5 as worded: 1024 -> 128 per GPU at N=8); 0 = weak scaling")
    ap.add_argument("--unique-scans", type=int, default=0, help="distinct scans generated per GPU; 0 = all (default). Fewer are tiled "
                    "to the batch and the JSON line says so")
    ap.add_argument("--map-warm", type=int, default=20, help="warm-up scans that build the shared map (SURVEY 8d: K0 = 20)")
    ap.add_argument("--stream-scans", type=int, default=24, help="consecutive scans of the single-stream (config 3) measurement")
    ap.add_argument("--cpu-sample", type=int, default=240, help="scans the oracle replays for cpu_baseline and parity_check (0 = skip)")
    ap.add_argument("--config1-overlay-repeat", type=int, default=3, help="replays of the config-1 batch WITH insert (the last one is timed; all must give the same bits)")
    ap.add_argument("--config1-scans", type=int, default=2048, help="scans of the ragged config-1 batch measured as an extra (0 = skip)")
    ap.add_argument("--sustained-s", type=float, default=1.2, help="length of the sustained run reported in extra (0 = skip)")
    ap.add_argument("--no-pcie", action="store_true", help="skip the host-resident (PCIe-inclusive) variant of the step")
    ap.add_argument("--shuffle-check", type=int, default=24, help="extra.shuffled_in_bucket_*: the same batch with a random permutation inside every time bucket (curvature kept) - "
                    "the headline's scans come in voxel-grid cell order inside a bucket; this many of its scans are replayed by the oracle (0 = skip the extra)")
    ap.add_argument("--shuffle-main", action="store_true", help="profiling aid: the MAIN timed loop runs on the batch with a random permutation inside every bucket "
                    "(tools/gpu_prof_shuffled.sh collects the residual kernel's counters for that order -> profiles/latest_shuffled_pmc.json); the line says so")
    ap.add_argument("--overlay-scans", type=int, default=1024, help="scans of the batch replayed WITH the map insert (per-scan overlay, extra.overlay_*; 0 = skip)")
    ap.add_argument("--config4-scans", type=int, default=100, help="extra.config4_*: consecutive Ouster-shaped scans (diter.yaml, 64 x 1024 rays, 500 Hz kinematic + IMU messages, leg "
                    "fusion) through decode -> voxel grid + time sort -> the live path with insert (BASELINE config 4; 0 = skip)")
    ap.add_argument("--config2-scans", type=int, default=256, help="extra.config2_*: scans of the batch whose residual ROWS are materialised in HBM in one launch (BASELINE config 2 "
                    "at bandwidth size: lk_batch_residuals_dev; 0 = skip)")
    ap.add_argument("--config2-check", type=int, default=4, help="of those, scans whose rows the oracle's residual build checks (valid mask, h / z / R)")
    ap.add_argument("--overlay-check", type=int, default=24, help="of those, scans the oracle replays (insert on, private copy of the map) for extra.overlay_parity")
    ap.add_argument("--max-roots-log2", type=int, default=15, help="root-voxel capacity (hash table = 8x, 16 B/slot)")
    ap.add_argument("--in-flight", type=int, default=2, help="batches in flight in the timed loop (slot ranges / streams they rotate over: 2 or 3; 3 gains 2 % in steady state - 1.753 vs 1.789 ms at 60 steps - and loses it to the longer drain of a 20-step region)")
    ap.add_argument("--step-sweep", action="store_true", help="also time regions of 1..64 steps (extra.step_sweep_ms)")
    ap.add_argument("--gen-workers", type=int, default=0, help="processes generating the synthetic scans (0 = auto)")
    ap.add_argument("--cache-dir", default="", help="keep generated inputs here between runs of one session (profiling passes)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write what the last timed step delivered (every scan's "
                    "pose record and its slot's state record, float64) as DIR/<name>.npy, at most 64 MB (a seeded sample of the scans beyond that)")
    ap.add_argument("--full", action="store_true", help="also run every extra measurement and check after the timed steps: parity check and CPU baselines "
                    "(--cpu-sample), sustained run, 128-scan shard, shuffled order (--shuffle-check), kernel-event pass, overlay batch (--overlay-scans), "
                    "configs 1-4 (--config1-scans, --config2-scans, --stream-scans, --config4-scans), PCIe-inclusive step, state-record gather and, at N > 1, "
                    "the scatter + all-gather map transport.  Without it the options of those extras are ignored")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: launch the N ranks ourselves (one process per GPU, rendezvous on 127.0.0.1) - the same
        # command line under torch.distributed.run; rank 0 of that run prints the JSON line, its exit code is ours
        import socket
        import subprocess

        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world_size != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_size} (launch with --nproc-per-node {args.gpus}, or without a launcher: bench.py starts its own ranks)")
    strong = args.total_scans > 0
    if strong:
        g0, g1 = replay.shard_range(args.total_scans, rank, world_size)
        S_max = replay.shard_range(args.total_scans, 0, world_size)[1]
    else:
        g0, g1 = rank * args.scans_per_gpu, (rank + 1) * args.scans_per_gpu
        S_max = args.scans_per_gpu
    S = g1 - g0
    assert S >= 1, "fewer scans than GPUs"
    U = S if args.unique_scans <= 0 else min(args.unique_scans, S)

    P = config.LEG_FUSION
    traj = synth.Trajectory()
    t0 = 5.0
    warm_t = [t0 + 3.0 * k for k in range(args.map_warm)]       # 20 poses over the 60 s figure-eight
    t_after = 5.0

    # ---- generation (fork pool, before any GPU work); a plain run generates only the batch and the map's scans
    t_gen0 = time.time()
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    workers = args.gen_workers or max(1, min(64, ncpu // max(1, world_size)))
    jobs = [("dense", (scan_time(t_after, g0 + u), N_BUCKETS, 5005 + g0 + u, 1_000_003 + g0 + u)) for u in range(U)]
    n_batch_jobs = len(jobs)
    ns = args.stream_scans if (rank == 0 and args.full) else 0
    n51 = max(3, min(ns, 6)) if ns >= 2 else 0
    U1 = 8 if (rank == 0 and world_size == 1 and args.full and args.config1_scans > 0) else 0
    if rank == 0:
        jobs.append(("first", (t0,)))
        jobs += [("dense", (tb, N_BUCKETS, 2002 + k, 3003 + k)) for k, tb in enumerate(warm_t)]
    jobs += [("dense", (t_after + 0.1 * k, N_BUCKETS, 8008 + k, 8108 + k)) for k in range(ns)]
    jobs += [("dense", (t_after + 0.1 * (ns + k), 51, 8208 + k, 8308 + k)) for k in range(n51)]
    jobs += [("vlp", (t_after + 0.1 * k, 7007 + k)) for k in range(U1)]
    U4 = args.config4_scans if (rank == 0 and world_size == 1 and args.full) else 0
    if U4:
        jobs.append(("ouster", (T0_CONFIG4, 3999, True)))
        jobs += [("ouster", (T0_CONFIG4 + 0.1 * k, 4000 + k, False)) for k in range(U4)]
    # optional per-job cache (profiling passes of one session re-run this command many times)
    def cpath(j):
        return os.path.join(args.cache_dir, "lk_" + j[0] + "_" + "_".join(repr(v) for v in j[1]) + ".npy")

    if args.cache_dir:
        os.makedirs(args.cache_dir, exist_ok=True)
        missing = [j for j in jobs if not os.path.exists(cpath(j))]
        for j, arr in zip(missing, generate(missing, workers)):
            np.save(cpath(j), arr)
        gen = [np.load(cpath(j)) for j in jobs]
    else:
        gen = generate(jobs, workers)
    it = iter(gen)
    scans = [next(it) for _ in range(n_batch_jobs)]
    first = warm = None
    if rank == 0:
        first = next(it)
        warm = [next(it) for _ in warm_t]
    sscans = [next(it) for _ in range(ns)]
    s51 = [next(it) for _ in range(n51)]
    c1_scans = [next(it) for _ in range(U1)]
    c4_static = next(it) if U4 else None
    c4_msgs = [next(it) for _ in range(U4)]
    gen_s = time.time() - t_gen0
    off, dt = synth.buckets_of(scans[0])
    assert all(len(sc) == N_PTS for sc in scans)
    tile = np.arange(S) % U
    xs = np.stack([synth.initial_state(traj, scan_time(t_after, g0 + int(tile[s])), P, np.random.default_rng(9009 + g0 + s), 0.02, 0.5)
                   for s in range(S)])
    Ps = np.tile((1e-4 * np.eye(30)).reshape(1, 900), (S, 1))

    import torch

    dist = None
    if world_size > 1:
        import torch.distributed as dist

        # test hooks (tools/gpu_multirank_selftest.sh): several ranks on ONE GPU over gloo exercise the whole N>1 code
        # path on a single-GPU box; the driver's real runs use neither variable (RCCL, one GPU per rank)
        backend = os.environ.get("LEGKILO_BENCH_BACKEND", "nccl")
        if os.environ.get("LEGKILO_BENCH_SHARE_GPU") == "1":
            local_rank = 0
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    # capacities sized to the scene (a 40 x 30 x 8 m room has ~20 k root voxels)
    mr = args.max_roots_log2
    cfg = config.make_config(P, device_id=local_rank, n_slots=max(2, args.in_flight) * S_max, max_roots=1 << mr, max_nodes=1 << (mr + 1),
                             max_point_blocks=1 << 17, max_scan_points=1 << 17)
    g = binding.LegKiloHip(cfg)  # raises without the HIP library / a gfx950 device

    # ---- shared map: rank 0 builds, RCCL broadcast of the device blob over xGMI
    warnings = []
    t_map0 = time.time()
    if rank == 0:
        build_map(g, traj, P, first, warm, warm_t)
    else:
        g.init_process_cov_q()
    map_bytes, bsecs = replay.broadcast_map(g, dist, rank, world_size, dev, src=0, algo="broadcast")
    bcast_ms = bsecs * 1e3 if world_size > 1 else None
    bcast2_ms = None
    if world_size > 1 and args.full:
        # the same payload again as scatter + all-gather (all xGMI links of the root busy); a failure is REPORTED, never hidden
        try:
            _, s2 = replay.broadcast_map(g, dist, rank, world_size, dev, src=0, algo="scatter_allgather")
            bcast2_ms = s2 * 1e3
        except Exception as e:  # noqa: BLE001
            msg = f"scatter_allgather map broadcast FAILED on backend {dist.get_backend()}: {type(e).__name__}: {str(e)[:160]}"
            if dist.get_backend() == "nccl":   # the real transport (RCCL over xGMI): never fall back silently - fail the run
                print(msg, file=sys.stderr, flush=True)
                raise
            warnings.append(msg)
    n_roots, n_nodes, n_blocks = g.map_stats()
    map_build_s = time.time() - t_map0
    # the checker replays against EXACTLY this snapshot: exported now, before the stream extras (which insert) touch the map
    map_blob_for_oracle = g.map_export() if (rank == 0 and world_size == 1 and args.full and args.cpu_sample > 0) else None

    # ---- resident batch
    host_batch = np.stack([np.ascontiguousarray(sc).view(np.uint8).reshape(-1) for sc in scans])      # U x 1.6 MB
    d_unique = torch.from_numpy(host_batch).to(dev)
    d_batch = d_unique if U == S else d_unique[torch.from_numpy(tile).to(dev)].contiguous()
    assert d_batch.numel() == S * N_PTS * 16

    def shuffled_in_bucket(batch, seed):
        """The same scans with a random permutation inside every time bucket (curvature kept): [S, N_PTS, 4] int32 view, on the device."""
        pts_i = batch.view(torch.int32).view(S, N_PTS, 4)
        out_ = torch.empty_like(pts_i)
        gen_t = torch.Generator(device=dev)
        gen_t.manual_seed(seed)
        for b in range(len(dt)):
            a_, e_ = int(off[b]), int(off[b + 1])
            if e_ <= a_:
                continue
            perm = torch.rand((S, e_ - a_), device=dev, generator=gen_t).argsort(dim=1)
            out_[:, a_:e_] = torch.gather(pts_i[:, a_:e_], 1, perm[..., None].expand(-1, -1, 4))
            del perm
        return out_

    if args.shuffle_main:
        d_batch = shuffled_in_bucket(d_batch, 4242).view(torch.uint8).reshape(S, -1)
        warnings.append("--shuffle-main: the timed loop ran on the batch with a RANDOM order inside every bucket (profiling aid), not on the headline's cell order")
    d_x = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
    d_P = torch.from_numpy(np.ascontiguousarray(Ps)).to(dev)
    torch.cuda.synchronize()
    # once per loaded batch, like the upload above: the library puts every bucket of the batch into root-voxel order in a copy of its own
    # (lk_batch_prepare_dev; a caller who does not ask gets the same at the batch's third replay - lk_batch_order).  The order INSIDE a time bucket is
    # left open by the reference (KILO.cc:369); with this step `value` no longer depends on the order the generator happens to emit.
    g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S)
    g.synchronize()
    tpz = time.perf_counter()
    if args.shuffle_main:
        g.batch_order(0)   # profiling aid: the random order is what is to be measured - the library leaves the batch alone
    else:
        g.batch_prepare_dev(d_batch.data_ptr(), S, N_PTS, off)
    batch_prepare_ms = (time.perf_counter() - tpz) * 1e3

    # Batches are enqueued back to back (lk_batch_replay_async_dev), alternating between two sets of filter slots and two
    # streams so that the update kernels of one batch overlap the residual launches of the next: every step still delivers
    # its poses to the host - into a pinned ring, copied on the stream - but no step waits for the previous one's results;
    # the timed region ends with everything synchronised and, for N > 1, the poses of all steps all-gathered.
    pose_sz = _abi.pose_dtype().itemsize
    ring_rows = max(args.steps, args.warmup, 2)
    ring = torch.zeros((ring_rows, S_max * pose_sz), dtype=torch.uint8).pin_memory()   # S_max columns: equal bytes on every rank
    gathered = [None]

    def step(k, batch_ptr=None):
        g.batch_replay_async_dev(d_batch.data_ptr() if batch_ptr is None else batch_ptr, (k % max(2, args.in_flight)) * S_max, S, N_PTS, 0.0, off, dt, d_x36=d_x.data_ptr(),
                                 d_P900=d_P.data_ptr(), host_out_ptr=ring[k % ring_rows].data_ptr())

    def finish(k_steps):
        g.synchronize()
        if dist is not None:   # every step's poses of every rank, all-gathered as raw records; the result stays on the device
            gathered[0] = replay.gather_pose_bytes(dist, ring[:min(k_steps, ring_rows)], world_size, dev)

    def sync_all():
        g.synchronize()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    t_setup_s = time.time() - T_PROCESS0
    for k in range(args.ramp_steps):   # untimed: brings the clocks up (the sustained rate is what the timed region should see)
        step(k)
    finish(min(args.ramp_steps, ring_rows))
    for k in range(args.warmup):
        step(k)
    finish(args.warmup)
    sync_all()
    t_start = time.perf_counter()
    for k in range(args.steps):
        step(k)
    finish(args.steps)
    sync_all()
    elapsed = time.perf_counter() - t_start
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    timed_last = ring[(args.steps - 1) % ring_rows][: S * pose_sz].numpy().view(_abi.pose_dtype()).copy()   # what the timed loop delivered
    gather_ok = None
    if dist is not None and (args.full or args.dump_outputs):   # untimed: the gathered records are what every rank delivered (rank r's last step == its own ring row)
        rec = gathered[0].cpu().numpy().reshape(world_size, -1, S_max * pose_sz)
        mine = rec[rank, (args.steps - 1) % ring_rows, : S * pose_sz].view(_abi.pose_dtype())
        gather_ok = bool(np.array_equal(mine["pos"], timed_last["pos"]) and all(
            (rec[r, (args.steps - 1) % ring_rows].view(_abi.pose_dtype())["n_buckets"][:1] == N_BUCKETS).all() for r in range(world_size)))
    n_eff = float(timed_last["n_effect"].astype(np.float64).mean())
    total_scans = (args.total_scans if strong else S * world_size) * args.steps
    value = total_scans / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    if args.dump_outputs:   # untimed, before anything else replays into the slots of the last timed step
        last_slot = ((args.steps - 1) % max(2, args.in_flight)) * S_max
        xs_last, Ps_last = replay.gather_state_records(dist, g, last_slot, S, world_size, dev)
        if rank == 0:
            if dist is None:
                poses_last = timed_last
            else:   # every rank's records of its last step, in rank order (a rank's row holds its own shard's scans first)
                shards = [replay.shard_range(args.total_scans, r, world_size) if strong else (0, S) for r in range(world_size)]
                poses_last = np.concatenate([rec[r, (args.steps - 1) % ring_rows].view(_abi.pose_dtype())[: b - a] for r, (a, b) in enumerate(shards)])
            dump_outputs(args.dump_outputs, poses_last, xs_last.cpu().numpy(), Ps_last.cpu().numpy())
        del xs_last, Ps_last

    # ---- sustained run (>= 1 s of back-to-back steps; same loop, not the graded number)
    extra = {"full": args.full, "setup_s": round(t_setup_s, 2)}
    if args.full:
        # untimed: SURVEY 8(e)'s full per-scan result record - state 36 + covariance 900 - of the last batch in slots [0, S), gathered on
        # the device by one kernel (lk_batch_get_states_dev) and, for N > 1, all-gathered device to device over RCCL
        xs_all, Ps_all = replay.gather_state_records(dist, g, 0, S, world_size, dev)
        extra["state_records_gathered"] = int(xs_all.shape[0])
        extra["state_record_bytes_per_scan"] = 936 * 8
        extra["state_records_cov_finite"] = bool(torch.isfinite(Ps_all).all().item())
        del xs_all, Ps_all
    if args.full and args.sustained_s > 0:
        n_sus = max(4, int(math.ceil(args.sustained_s * 1e3 / ms_per_step)))
        sync_all()
        ts = time.perf_counter()
        for k in range(n_sus):
            step(k)
        finish(min(n_sus, ring_rows))
        sync_all()
        sus = time.perf_counter() - ts
        extra["sustained_scans_per_s"] = round((args.total_scans if strong else S * world_size) * n_sus / sus, 1)
        extra["sustained_steps"] = n_sus
        extra["sustained_seconds"] = round(sus, 3)

    # ---- the strong-scaling shard on ONE GPU: BASELINE config 5 at N = 8 gives every GPU 128 of the 1024 scans.  The same loop with
    # 128-scan batches (three in flight, rotating over three slot ranges / streams) - what a GPU of the 8-GPU run executes per step.
    if args.full and S >= 128:
        S8 = 128
        ring8 = max(1, min(3, (max(2, args.in_flight) * S_max) // S8))   # slot ranges the 128-scan batches rotate over (a 128-scan rank has 256 slots: two)

        def step8(k):
            g.batch_replay_async_dev(d_batch.data_ptr(), (k % ring8) * S8, S8, N_PTS, 0.0, off, dt, d_x36=d_x.data_ptr(), d_P900=d_P.data_ptr(),
                                     host_out_ptr=ring[k % ring_rows].data_ptr())
        n8 = 8 * max(args.steps, 10)
        for k in range(max(args.warmup, 6)):
            step8(k)
        sync_all()
        ts = time.perf_counter()
        for k in range(n8):
            step8(k)
        sync_all()
        t8 = (time.perf_counter() - ts) / n8
        extra["shard128_ms_per_step"] = round(t8 * 1e3, 4)
        extra["shard128_ps_per_point"] = round(t8 * 1e12 / (S8 * N_PTS), 2)
        extra["shard128_scans_per_s"] = round(S8 / t8, 1)
        extra["shard128_vs_full_batch_ps_ratio"] = round((t8 / (S8 * N_PTS)) / (elapsed / args.steps / (S * N_PTS)), 3)
        extra["shard128_note"] = ("128-scan batches = one GPU's share of config 5 at N = 8, three batches in flight on one GPU; the shard's 205 MB of scan points "
                                  "are re-read every step and fit the 256 MB Infinity Cache (as they would on each GPU of the 8-GPU run); the SAME loop over "
                                  "1024 distinct scans in 128-scan sub-batches is slower than one 1024-scan launch per bucket (2.18 vs 1.69 ms)")

    if args.step_sweep:   # diagnostic: fixed cost (ramp + drain) vs per-step cost of a timed region, elapsed(K) = a + b K
        sweep = {}
        for K in (1, 2, 4, 8, 16, 32, 64):
            sync_all()
            ts = time.perf_counter()
            for k in range(K):
                step(k)
            finish(min(K, ring_rows))
            sync_all()
            sweep[K] = round((time.perf_counter() - ts) * 1e3, 3)
        extra["step_sweep_ms"] = sweep

    # ---- input-order sensitivity: the SAME batch with a random permutation inside every time bucket.  The headline's scans come, inside a
    # bucket, in voxel-grid cell order (synth.dense_scan(layout="cell"): the order pcl::VoxelGrid leaves its output in, KILO.cc:356-360), which
    # puts neighbouring lanes into neighbouring voxels; a recorded scan that was not voxel-filtered has no such order.
    shuf = None
    shuf_auto = None
    resorted = None
    if rank == 0 and world_size == 1 and args.full and args.shuffle_check > 0 and not args.shuffle_main:
        d_shuf = shuffled_in_bucket(d_batch, 4242)
        torch.cuda.synchronize()
        g.batch_order(0)   # LK_BATCH_ORDER_AS_GIVEN: what the random order costs when the library is told to leave the batch alone
        for k in range(max(args.warmup, 3)):
            step(k, d_shuf.data_ptr())
        finish(min(max(args.warmup, 3), ring_rows))
        sync_all()
        ts = time.perf_counter()
        for k in range(args.steps):
            step(k, d_shuf.data_ptr())
        finish(args.steps)
        sync_all()
        el_sh = time.perf_counter() - ts
        sh_last = ring[(args.steps - 1) % ring_rows][: S * pose_sz].numpy().view(_abi.pose_dtype()).copy()
        n_sh = min(args.shuffle_check, S)
        sh_host = d_shuf[:n_sh].cpu().numpy().view(scans[0].dtype).reshape(n_sh, N_PTS)
        extra["shuffled_in_bucket_ms_per_step"] = round(el_sh / args.steps * 1e3, 3)
        extra["shuffled_in_bucket_ps_per_point"] = round(el_sh / args.steps / N_BUCKETS * 1e12 / pts_per_launch_of(S), 2)
        extra["shuffled_in_bucket_scans_per_s"] = round(S * args.steps / el_sh, 1)
        extra["shuffled_in_bucket_over_cell_order"] = round((el_sh / args.steps) / (elapsed / args.steps), 3)
        extra["shuffled_in_bucket_mean_n_effect"] = float(sh_last["n_effect"].astype(np.float64).mean())
        pmc_sh = os.path.join(ROOT, "profiles", "latest_shuffled_pmc.json")
        if os.path.exists(pmc_sh):
            try:
                j_ = json.load(open(pmc_sh))
                extra["shuffled_in_bucket_tcc_req_per_point"] = j_.get("tcc_req_per_point")
                extra["shuffled_in_bucket_hbm_bytes_per_point"] = j_.get("hbm_bytes_per_point")
                extra["shuffled_in_bucket_pmc_source"] = f"profiles/latest_shuffled_pmc.json (tag {j_.get('tag')}, commit {j_.get('commit')})"
            except Exception as e:  # noqa: BLE001
                warnings.append(f"profiles/latest_shuffled_pmc.json unreadable: {e}")
        shuf = (sh_host, sh_last)
        g.batch_order(1)
        # ... and the SAME buffer under the library's default (LK_BATCH_ORDER_AUTO), nothing prepared by the caller: the first replays run as given, the
        # third makes the voxel-ordered copy (inside the warm-up steps), the timed steps read it
        try:
            g.batch_changed()
            n_warm_auto = max(args.warmup, 8)
            for k in range(n_warm_auto):
                step(k, d_shuf.data_ptr())
            finish(min(n_warm_auto, ring_rows))
            sync_all()
            ts = time.perf_counter()
            for k in range(args.steps):
                step(k, d_shuf.data_ptr())
            finish(args.steps)
            sync_all()
            el_au = time.perf_counter() - ts
            au_last = ring[(args.steps - 1) % ring_rows][: S * pose_sz].numpy().view(_abi.pose_dtype()).copy()
            extra["shuffled_auto_ms_per_step"] = round(el_au / args.steps * 1e3, 3)
            extra["shuffled_auto_over_headline"] = round((el_au / args.steps) / (elapsed / args.steps), 3)
            extra["shuffled_auto_order_stats"] = dict(zip(("examined", "sorted", "stale"), g.batch_order_stats()))
            shuf_auto = (sh_host, au_last)
        except Exception as e:  # noqa: BLE001
            extra["shuffled_auto_error"] = f"{type(e).__name__}: {str(e)[:160]}"
            warnings.append("auto-ordered replay of the shuffled batch failed: " + extra["shuffled_auto_error"])
        # ... and what it costs to put such a batch back into voxel order on the device (lk_batch_sort_by_voxel_dev: root-voxel key under the slot's
        # PRIOR pose, stable segmented radix sort of every bucket, one gather; once per loaded batch, not per replay), and the step on it
        try:
            g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S)
            d_res = torch.empty_like(d_shuf)
            g.batch_sort_by_voxel_dev(d_shuf.data_ptr(), d_res.data_ptr(), S, N_PTS, off)   # warm (allocations, rocPRIM's first call)
            torch.cuda.synchronize()
            ts = time.perf_counter()
            g.batch_sort_by_voxel_dev(d_shuf.data_ptr(), d_res.data_ptr(), S, N_PTS, off)
            torch.cuda.synchronize()
            t_sort = time.perf_counter() - ts
            for k in range(max(args.warmup, 3)):
                step(k, d_res.data_ptr())
            finish(min(max(args.warmup, 3), ring_rows))
            sync_all()
            ts = time.perf_counter()
            for k in range(args.steps):
                step(k, d_res.data_ptr())
            finish(args.steps)
            sync_all()
            el_rs = time.perf_counter() - ts
            rs_last = ring[(args.steps - 1) % ring_rows][: S * pose_sz].numpy().view(_abi.pose_dtype()).copy()
            n_rs = min(max(args.shuffle_check // 3, 1), S)
            rs_host = d_res[:n_rs].cpu().numpy().view(scans[0].dtype).reshape(n_rs, N_PTS)
            resorted = (rs_host, rs_last)
            extra["shuffled_resort_by_voxel_ms_per_batch_once"] = round(t_sort * 1e3, 2)
            extra["shuffled_resort_ps_per_point"] = round(t_sort * 1e12 / (S * N_PTS), 1)
            extra["shuffled_resort_entry"] = "lk_batch_sort_by_voxel_dev"
            extra["shuffled_resorted_ms_per_step"] = round(el_rs / args.steps * 1e3, 3)
            extra["shuffled_resort_breaks_even_after_steps"] = None if el_sh <= el_rs else int(math.ceil(t_sort / ((el_sh - el_rs) / args.steps)))
            del d_res
        except Exception as e:  # noqa: BLE001
            extra["shuffled_resort_error"] = f"{type(e).__name__}: {str(e)[:160]}"
            warnings.append("device re-sort of the shuffled batch failed: " + extra["shuffled_resort_error"])
        del d_shuf

    # ---- kernel-level timing pass (HIP events on the handle's stream, whole-batch launches on ONE stream), outside the timed region
    prof = None
    if args.full:
        g.profile_reset()
        g.profile_enable(1)
        g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S)
        g.batch_replay_dev(d_batch.data_ptr(), S, N_PTS, 0.0, off, dt)
        g.profile_enable(0)
        prof = {k: g.profile_get(k) for k in ("predict", "residual", "update")}
    pts_per_launch = S * (N_PTS // N_BUCKETS)
    # the launch time the roofline uses comes from the TIMED region: one step = N_BUCKETS residual launches with everything
    # else (update / predict / priors / pose copies) hidden under them or charged to them
    launch_ms = ms_per_step / N_BUCKETS
    pmc = None
    if os.path.exists(PMC_FILE):
        try:
            pmc = json.load(open(PMC_FILE))
        except Exception as e:  # noqa: BLE001
            warnings.append(f"profiles/latest_pmc.json unreadable: {e}")
    if pmc and pmc.get("kernel_sources_sha16") != kernel_sources_sha16():
        warnings.append(f"roofline counters (profiles/latest_pmc.json, tag {pmc.get('tag')}, commit {pmc.get('commit')}) were collected on a different "
                        f"version of {', '.join(KERNEL_SOURCES)}: re-run tools/gpu_prof_r03.sh")
    hbm_bpp = pmc.get("hbm_bytes_per_point") if pmc else None
    fp64_flops = pmc.get("fp64_flops_per_point") * pts_per_launch if pmc and pmc.get("fp64_flops_per_point") else None
    fp64_tflops = fp64_flops / (launch_ms * 1e-3) / 1e12 if fp64_flops else None
    traffic = hbm_bpp * pts_per_launch if hbm_bpp else None
    hbm_GBs = traffic / (launch_ms * 1e-3) / 1e9 if traffic else None
    l2_GBs = pmc["tcc_req_per_point"] * 128.0 * pts_per_launch / (launch_ms * 1e-3) / 1e9 if pmc and pmc.get("tcc_req_per_point") else None
    valu_frac = (pmc["valu_insts_per_wave"] * 4.0 * (pts_per_launch / 64.0) / (SIMDS * CLK_GHZ * 1e9 * launch_ms * 1e-3)
                 if pmc and pmc.get("valu_insts_per_wave") else None)
    # the same with the issue cost of each instruction class on a SIMD-16 pipe: 4 cycles per fp64 wave instruction (half rate), 2 per other VALU
    fp64_pw = pmc.get("fp64_insts_per_wave") if pmc else None
    valu_frac_class = (((fp64_pw * 4.0 + (pmc["valu_insts_per_wave"] - fp64_pw) * 2.0) * (pts_per_launch / 64.0) / (SIMDS * CLK_GHZ * 1e9 * launch_ms * 1e-3))
                       if pmc and fp64_pw and pmc.get("valu_insts_per_wave") else None)
    alg_GBs = ALG_BYTES_RESIDUAL * pts_per_launch / (launch_ms * 1e-3) / 1e9
    roofline = {
        "kernel": "lk_residual_kernel<false>",
        # what the counters say bounds it: fp64 VALU issue + dependent L2 round trips (56 % of wave life in s_waitcnt); the map is
        # L2 / MALL resident, HBM only carries the 16 B/point scan read and the 4 B/point partial records
        "bound": "valu_issue+l2_latency", "contract_bound": "hbm",
        "achieved": None if hbm_GBs is None else round(hbm_GBs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": None if hbm_GBs is None else round(hbm_GBs / HBM_PEAK_GBS, 4),
        "traffic": None if traffic is None else round(traffic),
        "hbm_frac_counters": None if hbm_GBs is None else round(hbm_GBs / HBM_PEAK_GBS, 4),
        "hbm_bytes_per_point_counters": hbm_bpp,
        "l2_GBs": None if l2_GBs is None else round(l2_GBs, 1), "l2_frac": None if l2_GBs is None else round(l2_GBs / L2_PEAK_GBS, 4),
        "valu_issue_frac": None if valu_frac is None else round(valu_frac, 3),
        "valu_issue_frac_by_class": None if valu_frac_class is None else round(valu_frac_class, 3),
        "valu_issue_cost_model": "valu_issue_frac charges 4 cycles to every VALU wave instruction; _by_class charges 4 to fp64 (half rate on the 16-lane pipe) and 2 to the others",
        # the roofline the kernel lives on: fp64 vector FLOP/s (counter-derived: 2 FMA + ADD + MUL + TRANS wave instructions x 64 lanes)
        "fp64_flops": None if fp64_flops is None else round(fp64_flops), "fp64_TFLOPs": None if fp64_tflops is None else round(fp64_tflops, 2),
        "fp64_peak_TFLOPs": FP64_PEAK_TFLOPS, "fp64_frac": None if fp64_tflops is None else round(fp64_tflops / FP64_PEAK_TFLOPS, 4),
        "fp64_flops_per_point": pmc.get("fp64_flops_per_point") if pmc else None,
        "compulsory_bytes_per_point": COMPULSORY_BYTES_PER_POINT,
        "traffic_over_compulsory": None if hbm_bpp is None else round(hbm_bpp / COMPULSORY_BYTES_PER_POINT, 3),
        "valu_insts_per_wave": pmc.get("valu_insts_per_wave") if pmc else None,
        "mfma_f64_ops": pmc.get("mfma_f64_ops") if pmc else None,
        "pmc_source": None if not pmc else f"profiles/latest_pmc.json (tag {pmc.get('tag')}, commit {pmc.get('commit')}, {pmc.get('slots')} slots x {pmc.get('unique_scans')} unique scans)",
        "launch_ms": round(launch_ms, 4), "launch_ms_source": f"timed region: ms_per_step / {N_BUCKETS} residual launches",
        "points_per_launch": pts_per_launch, "ps_per_point": round(launch_ms * 1e9 / pts_per_launch, 2),
        # algorithmic bytes served mostly by L2/MALL - NOT an HBM fraction (at SURVEY's 288 B/point it would exceed the peak)
        "alg_bytes_per_point": ALG_BYTES_RESIDUAL, "alg_GBs_cache_served": round(alg_GBs, 1),
        "survey_alg_bytes_per_point": ALG_BYTES_SURVEY, "alg_GBs_cache_served_at_survey_bytes": round(alg_GBs * ALG_BYTES_SURVEY / ALG_BYTES_RESIDUAL, 1),
    }
    if prof is not None:   # --full: the event pass's per-launch times
        roofline["launch_ms_single_stream_events"] = round(prof["residual"][1] / max(prof["residual"][0], 1), 4)
        roofline["launches_event_pass"] = prof["residual"][0]
        roofline["other_kernels_ms"] = {k: round(v[1] / max(v[0], 1), 4) for k, v in prof.items() if k != "residual"}
    # where the kernel's waves wait: L1 / LDS / SQ counters of the same launch, profiles/r06_pmc_memory_pipe.json (tools/gpu_prof_mempipe.sh)
    mp_file = os.path.join(ROOT, "profiles", "r06_pmc_memory_pipe.json")
    if os.path.exists(mp_file):
        try:
            mp = json.load(open(mp_file))
            dv = mp.get("cell", {}).get("derived", {})
            waves_per_simd = 5
            roofline["memory_pipe"] = {
                "source": f"profiles/r06_pmc_memory_pipe.json (commit {mp.get('commit')})" + ("" if mp.get("kernel_sources_sha16") == kernel_sources_sha16() else " - STALE: kernel sources changed since"),
                "wave_parked_frac": dv.get("sq_wait_any_frac_of_wave_cycles"), "wave_issue_stall_frac": dv.get("sq_wait_inst_any_frac_of_wave_cycles"),
                "wave_executing_frac": dv.get("sq_active_inst_any_frac_of_wave_cycles"), "wave_valu_executing_frac": dv.get("sq_active_inst_valu_frac_of_wave_cycles"),
                "vector_pipe_busy_at_5_waves_per_simd": None if dv.get("sq_active_inst_valu_frac_of_wave_cycles") is None else round(waves_per_simd * dv["sq_active_inst_valu_frac_of_wave_cycles"], 3),
                "l1_hit_rate": dv.get("tcp_l1_hit_rate"), "l1_miss_to_l2_latency_cycles": dv.get("tcp_read_req_to_l2_latency_cycles"),
                "l1_pending_stall_cycles_per_access": dv.get("tcp_pending_stall_cycles_per_cache_access"),
                "lds_bank_conflict_cycles_per_lds_cycle": dv.get("lds_bank_conflict_cycles_per_lds_active_cycle"),
                "tlb_misses_per_point": dv.get("utcl1_translation_misses_per_point"),
                "verdict": "bound by fp64 VALU issue: every wave is parked ~47 % of its life, but five waves per SIMD keep the vector pipe ~0.87 busy; L1 hit rate 0.9, "
                           "~290 cycles per L1 miss to L2, negligible L1 stall / tag-conflict / LDS-conflict / TLB shares - the memory pipe is not the limit "
                           "(TA_* / TD_* counters cannot be collected on this pool: rocprofv3 never completes the first dispatch)",
            }
            roofline["bound"] = "fp64_valu_issue (memory pipe measured: not the limit)"
        except Exception as e:  # noqa: BLE001
            warnings.append(f"profiles/r06_pmc_memory_pipe.json unreadable: {e}")

    # ---- extra: the same batch WITH the map insert - every scan on its own copy-on-write overlay of the shared map (SURVEY 8d config 5,
    # "scan-local insert overlay"; KILO.cc:216-233 after every bucket): what KILO::process computes per scan, for the whole batch
    ov = None
    S_ov = min(args.overlay_scans, S) if args.full else 0   # every rank replays its own shard with insert (an overlay is private to its scan: no collective on the data path)
    if S_ov > 0:
        try:
            g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S_ov)
            g.batch_replay_overlay_dev(d_batch.data_ptr(), S_ov, N_PTS, 0.0, off, dt, want_poses=False)   # warm (allocates the overlay pools)
            g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S_ov)
            g.batch_replay_overlay_dev(d_batch.data_ptr(), S_ov, N_PTS, 0.0, off, dt, want_poses=False)   # second warm run: pools re-made at the first run's high-water marks + 25 %
            tov = []
            for _ in range(3):
                g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S_ov)
                sync_all()                                  # N > 1: every rank starts its batch together, the slowest rank's time counts
                tc = time.perf_counter()
                ov_poses = g.batch_replay_overlay_dev(d_batch.data_ptr(), S_ov, N_PTS, 0.0, off, dt)
                t_one = time.perf_counter() - tc
                if dist is not None:
                    tt = torch.tensor([t_one], dtype=torch.float64, device=dev)
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    t_one = float(tt.item())
                tov.append(t_one)
            t_ov = float(np.median(tov))
            ov_p = np.frombuffer(ov_poses, dtype=_abi.pose_dtype()).copy()
            S_ov_all = S_ov
            if dist is not None:   # shards may differ by one scan in the strong-scaling mode
                tt = torch.tensor([S_ov], dtype=torch.int64, device=dev)
                dist.all_reduce(tt, op=dist.ReduceOp.SUM)
                S_ov_all = int(tt.item())
                # the per-scan results of every rank's overlay batch, all-gathered (what a sharded replay returns: replay.replay_batch_overlay)
                rows_all = replay.gather_results(dist, replay.pose_rows(ov_p), world_size, dev)
                extra["overlay_rows_gathered"] = int(rows_all.shape[0])
            extra["overlay_scans"] = S_ov_all
            extra["overlay_scans_per_gpu"] = S_ov
            extra["overlay_ms_per_batch"] = round(t_ov * 1e3, 3)
            extra["overlay_scans_per_s"] = round(S_ov_all / t_ov, 1)
            # SURVEY 8(d)'s contract bytes (288 + 728 B per point entering the path), for reference only: half of the bench's points land in
            # frozen leaves and are dropped after one bit test (the reference ignores them too), so this is NOT an achieved HBM rate - the
            # counter-derived figure is extra.overlay_roofline
            extra["overlay_contract_bytes_for_reference"] = {"bytes_per_point": ALG_BYTES_FULL, "GBs_if_every_point_moved_them": round(ALG_BYTES_FULL * N_PTS * S_ov_all / t_ov / 1e9, 1)}
            extra["overlay_mean_n_effect"] = round(float(ov_p["n_effect"].astype(np.float64).mean()), 1)
            r_, n_, b_ = g.overlay_stats()
            extra["overlay_private_per_scan_max"] = {"roots": r_, "nodes": n_, "point_blocks": b_}
            pb_, pe_, pc_, pk_ = g.overlay_pool_bytes()
            extra["overlay_pool_bytes"] = int(pb_)
            extra["overlay_pool_per_scan"] = {"root_entries": pe_, "child_nodes": pc_, "point_blocks": pk_, "MB": round(pb_ / max(S_ov, 1) / 1e6, 1)}
            # where the time goes: the same replay once more with an event pair around every launch
            g.profile_reset()
            g.profile_enable(1)
            g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S_ov)
            g.batch_replay_overlay_dev(d_batch.data_ptr(), S_ov, N_PTS, 0.0, off, dt, want_poses=False)
            g.profile_enable(0)
            extra["overlay_kernel_ms_per_batch"] = {k: round(g.profile_get(k)[1], 3) for k in OV_KERNELS if g.profile_get(k)[0]}
            extra["overlay_roofline"] = overlay_roofline(extra["overlay_kernel_ms_per_batch"], {k: g.profile_get(k)[0] for k in OV_KERNELS}, S_ov, warnings)
            ov = ov_p
        except Exception as e:  # noqa: BLE001
            extra["overlay_error"] = f"{type(e).__name__}: {str(e)[:300]}"
            warnings.append("overlay replay failed: " + extra["overlay_error"])

    # ---- extra: BASELINE config 2 ("100k-pt scan, voxel kNN + point-to-plane residuals only vs CPU") at bandwidth size: the residual build
    # of KILO.cc:122-210 for S2 x 100 000 points in ONE launch, every scan under its prior state, rows h (1x6) / z / R / valid MATERIALISED in
    # HBM (lk_batch_residuals_dev).  This is the one place SURVEY 8(d)'s HBM roofline applies as written: 16 B in + 65 B out per point.
    c2 = None
    S2 = min(args.config2_scans, S) if (rank == 0 and world_size == 1 and args.full) else 0
    if S2 > 0:
        try:
            N2 = S2 * N_PTS
            d_rows = torch.empty((N2, 8), dtype=torch.float64, device=dev)   # per point: h (1 x 6), z, R
            d_v = torch.empty(N2, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def run_c2():
                g.batch_residuals_dev(d_batch.data_ptr(), S2, N_PTS, d_rows.data_ptr(), d_v.data_ptr())

            g.batch_set_priors_dev(d_x.data_ptr(), d_P.data_ptr(), S2)
            for _ in range(3):
                run_c2()
            g.synchronize()
            K2 = 10
            ts = time.perf_counter()
            for _ in range(K2):
                run_c2()
            g.synchronize()
            t_c2 = (time.perf_counter() - ts) / K2
            g.profile_reset()
            g.profile_enable(1)     # HIP events around the launch, on the handle's stream
            for _ in range(5):
                run_c2()
            g.profile_enable(0)
            n_ev, ms_ev = g.profile_get("residual_rows")
            ev_ms = ms_ev / max(n_ev, 1)
            n_chk2 = min(args.config2_check, S2)
            r8 = d_rows[:n_chk2 * N_PTS].cpu().numpy()
            c2 = (np.ascontiguousarray(r8[:, :6]), np.ascontiguousarray(r8[:, 6]), np.ascontiguousarray(r8[:, 7]), d_v[:n_chk2 * N_PTS].cpu().numpy())
            matched = float(d_v.to(torch.float32).mean().item())
            del d_rows, d_v, r8
            c2pmc = None
            if os.path.exists(C2_PMC_FILE):
                c2pmc = json.load(open(C2_PMC_FILE))
                if c2pmc.get("kernel_sources_sha16") != kernel_sources_sha16():
                    warnings.append(f"config-2 counters (profiles/latest_config2_pmc.json, tag {c2pmc.get('tag')}) were collected on a different version of "
                                    f"{', '.join(KERNEL_SOURCES)}: re-run tools/gpu_prof_config2.sh")
            else:
                warnings.append("profiles/latest_config2_pmc.json missing: extra.config2_roofline has no counter-derived traffic (tools/gpu_prof_config2.sh)")
            hbm2 = c2pmc.get("hbm_bytes_per_point") if c2pmc else None
            extra["config2_scans"] = S2
            extra["config2_points_per_launch"] = N2
            extra["config2_ms_per_launch"] = round(t_c2 * 1e3, 4)
            extra["config2_ps_per_point"] = round(t_c2 * 1e12 / N2, 2)
            extra["config2_scans_per_s"] = round(S2 / t_c2, 1)
            extra["config2_matched_fraction"] = round(matched, 4)
            extra["config2_roofline"] = {
                "kernel": "lk_residual_kernel<true> (rows emitted)", "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "launch_ms_events": round(ev_ms, 4), "launch_ms_wall": round(t_c2 * 1e3, 4), "launches_event_pass": n_ev,
                "alg_bytes_per_point": C2_BYTES_PER_POINT, "achieved": round(C2_BYTES_PER_POINT * N2 / (ev_ms * 1e-3) / 1e9, 1),
                "frac": round(C2_BYTES_PER_POINT * N2 / (ev_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "frac_of_copy_ceiling": round(C2_BYTES_PER_POINT * N2 / (ev_ms * 1e-3) / 1e9 / HBM_COPY_CEILING_GBS, 4),
                "traffic": None if hbm2 is None else round(hbm2 * N2),
                "hbm_bytes_per_point_counters": hbm2,
                "achieved_counters_GBs": None if hbm2 is None else round(hbm2 * N2 / (ev_ms * 1e-3) / 1e9, 1),
                "frac_counters": None if hbm2 is None else round(hbm2 * N2 / (ev_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "traffic_over_algorithmic": None if hbm2 is None else round(hbm2 / C2_BYTES_PER_POINT, 3),
                "pmc_source": None if not c2pmc else f"profiles/latest_config2_pmc.json (tag {c2pmc.get('tag')}, commit {c2pmc.get('commit')}, {c2pmc.get('slots')} slots)",
                "valu_insts_per_wave": c2pmc.get("valu_insts_per_wave") if c2pmc else None,
                "wait_any_frac_of_wave_cycles": c2pmc.get("wait_any_frac_of_wave_cycles") if c2pmc else None,
            }
        except Exception as e:  # noqa: BLE001
            extra["config2_error"] = f"{type(e).__name__}: {str(e)[:300]}"
            warnings.append("config-2 rows launch failed: " + extra["config2_error"])

    extra["ramp_steps_before_warmup"] = args.ramp_steps
    extra["batch_prepare_ms_once"] = round(batch_prepare_ms, 2)
    extra["batch_order_stats"] = dict(zip(("examined", "sorted", "stale"), g.batch_order_stats()))
    extra.update({"map_bytes": int(map_bytes), "map_roots": n_roots, "map_nodes": n_nodes, "map_build_s": round(map_build_s, 2),
                  "generate_s": round(gen_s, 1), "gen_workers": workers, "mean_n_effect": n_eff, "pose_gather_ok": gather_ok,
                  # the transport the two timings belong to: "nccl" = RCCL over xGMI (one GPU per rank - the driver's multi-GPU runs); "gloo" = the
                  # single-box self-test hook (LEGKILO_BENCH_BACKEND=gloo: several ranks share one GPU, the collectives go through host memory)
                  "collective_backend": None if dist is None else str(dist.get_backend()),
                  "map_broadcast_ms": bcast_ms, "map_scatter_allgather_ms": bcast2_ms,
                  "ranks_sharing_one_gpu": bool(os.environ.get("LEGKILO_BENCH_SHARE_GPU") == "1") if dist is not None else None})
    # ---- extra: the same batch step when the scans start in (pinned) host memory: upload of batch k+1 on a copy stream under
    # the replay of batch k (the boundary also takes host buffers; this rate is never `value`)
    if rank == 0 and world_size == 1 and args.full and not args.no_pcie:
        try:
            h_batch = torch.empty(d_batch.shape, dtype=d_batch.dtype).pin_memory()
            h_batch.copy_(d_batch)
            bufs = [d_batch, torch.empty_like(d_batch)]
            cs = torch.cuda.Stream()
            with torch.cuda.stream(cs):
                bufs[1].copy_(h_batch, non_blocking=True)
            cs.synchronize()
            t_p = time.perf_counter()
            KP = 3
            for k in range(KP):
                with torch.cuda.stream(cs):
                    bufs[(k + 1) & 1].copy_(h_batch, non_blocking=True)
                g.batch_replay_async_dev(bufs[k & 1].data_ptr(), (k & 1) * S_max, S, N_PTS, 0.0, off, dt, d_x36=d_x.data_ptr(),
                                         d_P900=d_P.data_ptr(), host_out_ptr=ring[0].data_ptr())
                g.synchronize()
                cs.synchronize()
            t_p = (time.perf_counter() - t_p) / KP
            extra["pcie_inclusive_scans_per_s"] = round(S / t_p, 1)
            extra["pcie_inclusive_ms_per_step"] = round(t_p * 1e3, 3)
            extra["pcie_h2d_GBs"] = round(d_batch.numel() / t_p / 1e9, 1)
            del h_batch, bufs
        except Exception as e:   # host memory for the pinned copy may be short on some boxes
            extra["pcie_inclusive_error"] = str(e)[:120]
    # ---- extra: a recorded-run shaped batch - the reference's own configuration (config 1: VLP-16 scans, voxel-grid
    # filtered to a few thousand points, 2 ms time bins -> hundreds of small buckets per scan, every scan with its own
    # tables and start time) through the ragged entry, all 2 x S filter slots in one batch, frozen map
    c1 = None
    if U1:
        c1_tb = [t_after + 0.1 * k for k in range(U1)]
        S1 = min(args.config1_scans, 2 * S_max)
        tile1 = np.arange(S1) % U1
        rng1 = np.random.default_rng(7107)
        xs1 = np.stack([synth.initial_state(traj, c1_tb[u], P) for u in tile1])
        xs1[:, 9:12] += rng1.normal(0, 0.005, (S1, 3))
        Ps1 = np.tile((1e-4 * np.eye(30)).reshape(1, 900), (S1, 1))
        tabs = [synth.buckets_of(sc_) for sc_ in c1_scans]
        scan_off = np.r_[0, np.cumsum([len(c1_scans[u]) for u in tile1])]
        allp = np.ascontiguousarray(np.concatenate([c1_scans[u] for u in tile1]))
        d_c1 = torch.empty(allp.nbytes, dtype=torch.uint8, device=dev)
        g.h2d(d_c1.data_ptr(), allp)
        d_x1, d_P1 = torch.from_numpy(xs1).to(dev), torch.from_numpy(Ps1).to(dev)
        offs, dts, tbs1 = [tabs[u][0] for u in tile1], [tabs[u][1] for u in tile1], [c1_tb[u] for u in tile1]
        tables1 = g.ragged_tables(scan_off, offs, dts, tbs1)   # once per recorded run

        def run_c1():
            g.batch_set_priors_dev(d_x1.data_ptr(), d_P1.data_ptr(), S1)
            return g.batch_replay_ragged_dev(d_c1.data_ptr(), tables1)

        run_c1()
        tc = time.perf_counter()
        for _ in range(3):
            poses1 = run_c1()
        el1 = (time.perf_counter() - tc) / 3
        p1 = np.frombuffer(poses1, dtype=_abi.pose_dtype())
        # the same batch with the bucket tables built on the device (lk_batch_replay_scans_dev): no host-side table work at all
        def run_c1_dev():
            g.batch_set_priors_dev(d_x1.data_ptr(), d_P1.data_ptr(), S1)
            return g.batch_replay_scans_dev(d_c1.data_ptr(), scan_off, tbs1)

        run_c1_dev()
        tc = time.perf_counter()
        for _ in range(3):
            poses1d = run_c1_dev()
        el1d = (time.perf_counter() - tc) / 3
        p1d = np.frombuffer(poses1d, dtype=_abi.pose_dtype())
        extra["config1_scans_dev_ms_per_batch"] = round(el1d * 1e3, 2)
        extra["config1_scans_dev_scans_per_s"] = round(S1 / el1d, 1)
        extra["config1_scans_dev_equals_host_tables"] = bool(np.array_equal(p1d["pos"], np.frombuffer(poses1, dtype=_abi.pose_dtype())["pos"]))
        extra["config1_ragged_scans_per_s"] = round(S1 / el1, 1)
        extra["config1_ragged_ms_per_batch"] = round(el1 * 1e3, 2)
        extra["config1_batch"] = int(S1)
        extra["config1_unique_scans"] = U1
        extra["config1_points_per_scan"] = round(float(len(allp)) / S1, 1)
        extra["config1_buckets_per_scan"] = round(float(p1["n_buckets"].mean()), 1)
        extra["config1_mean_n_effect"] = round(float(p1["n_effect"].astype(np.float64).mean()), 1)
        # the same recorded-run batch WITH the map insert, every scan on its own overlay (lk_batch_replay_overlay_ragged_dev: bucket index after
        # bucket index over all scans - the launches are what it costs)
        p1ov = None
        try:
            S1o = min(S1, S_max)
            tables1o = g.ragged_tables(scan_off[:S1o + 1], offs[:S1o], dts[:S1o], tbs1[:S1o])

            def run_c1_ov():
                g.batch_set_priors_dev(d_x1.data_ptr(), d_P1.data_ptr(), S1o)
                return g.batch_replay_overlay_ragged_dev(d_c1.data_ptr(), tables1o)

            first = bytes(run_c1_ov())
            same = 0
            for _ in range(max(1, args.config1_overlay_repeat - 2)):   # the same batch again: the same bits every time (the overlays start empty)
                same += int(bytes(run_c1_ov()) == first)
            tc = time.perf_counter()
            poses1o = run_c1_ov()
            el1o = time.perf_counter() - tc
            same += int(bytes(poses1o) == first)
            extra["config1_overlay_ragged_replays_identical"] = f"{same} / {max(1, args.config1_overlay_repeat - 2) + 1}"
            if same != max(1, args.config1_overlay_repeat - 2) + 1:
                warnings.append("config-1 overlay replay: a repeated replay of the same batch gave other results")
            p1ov = np.frombuffer(poses1o, dtype=_abi.pose_dtype()).copy()
            extra["config1_overlay_ragged_ms_per_batch"] = round(el1o * 1e3, 2)
            extra["config1_overlay_ragged_scans_per_s"] = round(S1o / el1o, 1)
            extra["config1_overlay_ragged_batch"] = int(S1o)
            extra["config1_overlay_ragged_mean_n_effect"] = round(float(p1ov["n_effect"].astype(np.float64).mean()), 1)
            # launches of the scan-resident kernel (1 + the most fallback stops of any scan); 0: the batch ran launch by launch (LEGKILO_RAG_RESIDENT=0, or a bucket over 512 points)
            extra["config1_overlay_ragged_resident_launches"] = g.overlay_resident_rounds()
            # counter-derived figures of that replay (tools/gpu_prof_ragov.sh -> profiles/latest_ragged_overlay_pmc.json), time from THIS run
            rr = {"bound": "latency: one wave per scan runs the scan's whole bucket chain - a dependent chain of wave instructions and memory round trips, not bandwidth",
                  "ms_per_batch": extra["config1_overlay_ragged_ms_per_batch"], "peak": HBM_PEAK_GBS, "unit": "GB/s"}
            if os.path.exists(RAGOV_PMC_FILE):
                rp = json.load(open(RAGOV_PMC_FILE))
                rr["pmc_source"] = f"profiles/latest_ragged_overlay_pmc.json (tag {rp.get('tag')}, commit {rp.get('commit')})"
                if rp.get("kernel_sources_sha16") != kernel_sources_sha16(RAGOV_KERNEL_SOURCES):
                    warnings.append(f"recorded-run overlay counters (profiles/latest_ragged_overlay_pmc.json, tag {rp.get('tag')}) were collected on a different version of "
                                    f"{', '.join(RAGOV_KERNEL_SOURCES)}: re-run tools/gpu_prof_ragov.sh")
                k = (rp.get("kernels") or {}).get("lk_rag_ov_scan_kernel")
                if k and extra["config1_overlay_ragged_resident_launches"]:
                    scans_prof = (rp.get("unprofiled_line") or {}).get("config1_overlay_ragged_batch") or S1o
                    rr.update({"kernel": "lk_rag_ov_scan_kernel", "launches_per_batch": k["launches_per_replay"], "kernel_ms_under_profiler": round(k["ms_per_replay"], 3),
                               "traffic": k["hbm_MB_per_replay"] * 1e6, "achieved": round(k["hbm_MB_per_replay"] * 1e6 / (el1o) / 1e9, 1),
                               "frac": round(k["hbm_MB_per_replay"] * 1e6 / el1o / 1e9 / HBM_PEAK_GBS, 4),
                               "valu_wave_insts_per_scan": round(k["valu_insts_per_replay"] / scans_prof), "wait_any_frac_of_wave_cycles": k["wait_any_frac_of_wave_cycles"]})
            else:
                rr["pmc_source"] = None
                warnings.append("profiles/latest_ragged_overlay_pmc.json missing: extra.config1_overlay_ragged_roofline has the time only (tools/gpu_prof_ragov.sh)")
            extra["config1_overlay_ragged_roofline"] = rr
        except Exception as e:  # noqa: BLE001
            extra["config1_overlay_ragged_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            warnings.append("config-1 overlay replay failed: " + extra["config1_overlay_ragged_error"])
        c1 = (c1_scans, c1_tb, xs1, Ps1, tile1, p1.copy(), p1ov)
        # live stream of ONE config-1 scan sequence (what a robot runs: bucket after bucket, with insert)
        g.set_state(synth.initial_state(traj, c1_tb[0], P), 1e-6 * np.eye(30), slot=0)
        g.set_times(c1_tb[0], c1_tb[0])
        tl = []
        for k in range(U1):
            tc = time.perf_counter()
            g.process_scan(c1_scans[k], c1_tb[k])
            tl.append(time.perf_counter() - tc)
        extra["config1_live_stream_ms_per_scan"] = round(float(np.median(tl[1:])) * 1e3, 3)
        del d_c1, d_x1, d_P1
    # ---- extra: BASELINE config 4 ("Diter++ Go2 sequence replay, IMU-as-observation + leg-kinematic factors, 1 MI355X"): no bag exists here, so
    # SURVEY 8(d)'s synthetic stand-in - diter.yaml, an Ouster-like 64 x 1024 message every 0.1 s, 500 Hz kinematic + IMU messages (trot
    # gait), only_imu_use: false - as a LIVE run on its own handle: per scan lk_decode_scan (lidar_processing.cc:54-80) -> lk_preprocess_scan
    # (pcl::VoxelGrid + time sort, KILO.cc:356-370) -> lk_process_scan (bucket loop with predictUpdateKinImu between the buckets, insert after
    # every bucket, KILO.cc:367-396), each timed on its own.  The CPU port and the reference's own build replay the same scans below.
    c4 = None
    if U4:
        try:
            P4 = config.DITER
            cfg4 = config.make_config(P4, device_id=local_rank, n_slots=1, max_roots=1 << 15, max_nodes=1 << 16, max_point_blocks=1 << 15, max_scan_points=1 << 17)
            g4 = binding.LegKiloHip(cfg4)
            x04 = synth.initial_state(traj, T0_CONFIG4, P4)
            g4.set_state(x04, 1e-6 * np.eye(30))
            g4.init_process_cov_q()
            g4.set_acc_norm(9.81)
            g4.set_times(T0_CONFIG4, T0_CONFIG4)
            dec0, _, _ = g4.decode_scan(c4_static.tobytes(), len(c4_static), OUSTER_MSG_LAYOUT, P4["time_scale"], P4["filter_num"], P4["blind"], header_stamp=T0_CONFIG4)
            xb4 = xyz_of(dec0)
            xw4 = world_of(x04, xb4, P4)
            g4.map_build(xw4, xb4)
            kins4 = [synth.kin_stream(traj, T0_CONFIG4 + 0.1 * k, T0_CONFIG4 + 0.1 * (k + 1), P4, seed=5000 + k) for k in range(U4)]
            t_dec, t_pre, t_path, ds4, tb4, poses4 = [], [], [], [], [], []
            for k in range(U4):
                msg = c4_msgs[k].tobytes()
                tb = T0_CONFIG4 + 0.1 * k
                tc = time.perf_counter()
                dec, b_, _ = g4.decode_scan(msg, len(c4_msgs[k]), OUSTER_MSG_LAYOUT, P4["time_scale"], P4["filter_num"], P4["blind"], header_stamp=tb)
                t1_ = time.perf_counter()
                ds = g4.preprocess_scan(dec, P4["voxel_grid_resolution"])
                t2_ = time.perf_counter()
                pose, _ = g4.process_scan(ds, b_, kins=kins4[k])
                t3_ = time.perf_counter()
                t_dec.append(t1_ - tc), t_pre.append(t2_ - t1_), t_path.append(t3_ - t2_)
                ds4.append(ds), tb4.append(b_)
                poses4.append((int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect), np.array(pose.pos), np.array(pose.rot)))
            rs4 = g4.stream_resident_stats()
            sk = slice(1, None)   # the first scan pays one-off allocations
            extra["config4_scans"] = U4
            extra["config4_points_per_message"] = round(float(np.mean([len(m) for m in c4_msgs])), 1)
            extra["config4_points_per_scan_after_voxel_grid"] = round(float(np.mean([len(d) for d in ds4])), 1)
            extra["config4_buckets_per_scan"] = round(float(np.mean([p_[0] for p_ in poses4])), 1)
            extra["config4_kin_imu_messages_per_scan"] = round(float(np.mean([len(k_) for k_ in kins4])), 1)
            extra["config4_mean_n_effect"] = round(float(np.mean([p_[2] for p_ in poses4])), 1)
            extra["config4_decode_ms_per_scan"] = round(float(np.median(t_dec[sk])) * 1e3, 3)
            extra["config4_preprocess_ms_per_scan"] = round(float(np.median(t_pre[sk])) * 1e3, 3)
            extra["config4_path_ms_per_scan"] = round(float(np.median(t_path[sk])) * 1e3, 3)
            extra["config4_path_scans_per_s"] = round(1.0 / float(np.median(t_path[sk])), 1)
            extra["config4_path_us_per_bucket"] = round(float(np.median(t_path[sk])) * 1e6 / max(1.0, extra["config4_buckets_per_scan"]), 2)
            extra["config4_all_three_ms_per_scan"] = round(float(np.median(np.array(t_dec[sk]) + np.array(t_pre[sk]) + np.array(t_path[sk]))) * 1e3, 3)
            extra["config4_resident_kernel_relaunches"] = int(rs4[1])
            extra["config4_note"] = ("host buffers in, pose out: every stage includes its PCIe copies and its synchronisation; `path` = the reference's timed lambda "
                                     "(KILO.cc:367-396: bucket loop with kinematic + IMU updates between the buckets and the map insert after every bucket)")
            c4 = (cfg4, x04, xw4, xb4, ds4, tb4, kins4, poses4)
            g4.close()
        except Exception as e:  # noqa: BLE001
            extra["config4_error"] = f"{type(e).__name__}: {str(e)[:300]}"
            warnings.append("config-4 live run failed: " + extra["config4_error"])
    cpu_baseline = None
    parity = None
    if rank == 0 and ns >= 2:
        g.set_state(synth.initial_state(traj, t_after, P), 1e-6 * np.eye(30), slot=0)
        g.set_times(t_after, t_after)
        d_s = torch.empty(ns * N_PTS * 16, dtype=torch.uint8, device=dev)
        g.h2d(d_s.data_ptr(), np.concatenate(sscans))
        g.process_scan_dev(d_s.data_ptr(), N_PTS, t_after, off, dt)  # warm
        g.synchronize()
        ts = time.perf_counter()
        for k in range(1, ns):
            g.process_scan_dev(d_s.data_ptr() + k * N_PTS * 16, N_PTS, t_after + 0.1 * k, off, dt)
        g.synchronize()
        stream_s = (time.perf_counter() - ts) / (ns - 1)
        extra["stream_scans_per_s"] = round(1.0 / stream_s, 1)
        extra["stream_ms_per_scan"] = round(stream_s * 1e3, 3)
        extra["stream_alg_GBs"] = round(ALG_BYTES_FULL * N_PTS / stream_s / 1e9, 1)
        # "... and report the 51-bucket variant" - the reference's own time quantisation
        # (2 ms bins of a 0.1 s scan, lidar_processing.cc:48): 51 predict / residual / update / insert cycles per scan
        off51, dt51 = synth.buckets_of(s51[0])
        same = all(np.array_equal(synth.buckets_of(sc_)[0], off51) for sc_ in s51)
        d_51 = torch.empty(n51 * N_PTS * 16, dtype=torch.uint8, device=dev)
        g.h2d(d_51.data_ptr(), np.concatenate(s51))

        def run51(k):
            o_, d_ = (off51, dt51) if same else synth.buckets_of(s51[k])
            g.process_scan_dev(d_51.data_ptr() + k * N_PTS * 16, N_PTS, t_after + 0.1 * (ns + k), o_, d_)
        run51(0)
        g.synchronize()
        ts = time.perf_counter()
        for k in range(1, n51):
            run51(k)
        g.synchronize()
        s51_s = (time.perf_counter() - ts) / (n51 - 1)
        extra["stream51_ms_per_scan"] = round(s51_s * 1e3, 3)
        extra["stream51_scans_per_s"] = round(1.0 / s51_s, 1)
        extra["stream51_buckets"] = int(len(dt51))
        sb, stl, srd = g.stream_stats()
        extra["stream_pipeline_stats"] = {"pipelined_buckets": sb, "tiles_verified": stl, "tiles_evaluated_again": srd}

    if rank == 0 and args.full and args.cpu_sample > 0 and world_size == 1:
        # ---- CPU baseline + in-line parity check: the oracle (port), 1 pinned thread, a bounded sample of the SAME batch on the
        # SAME map (the device's blob, imported into the oracle), compared with the poses the TIMED loop delivered
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_binding as ob

        try:
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[-1]})
        except Exception:
            pass
        o = ob.Oracle(cfg, imu_mode_only=True)
        o.init_process_cov_q()
        o.set_acc_norm(9.81)
        o.map_import(map_blob_for_oracle)
        o.set_map_insert(False)
        n_chk = min(args.cpu_sample, S)
        tcs, d_pos, d_rot, cnt_eq, worst = [], 0.0, 0.0, 0, None
        for s in range(n_chk):
            o.set_state(xs[s], Ps[s])
            o.set_times(0.0, 0.0)
            tc = time.perf_counter()
            pose, _ = o.process_scan(scans[tile[s]], 0.0, with_sort=True)
            tcs.append(time.perf_counter() - tc)
            tl_ = timed_last[s]
            same_counts = (int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect)) == (int(tl_["n_buckets"]), int(tl_["n_updates"]), int(tl_["n_effect"]))
            cnt_eq += int(same_counts)
            dp = float(np.abs(np.array(pose.pos) - tl_["pos"]).max())
            dr = float(np.abs(np.array(pose.rot) - tl_["rot"]).max())
            if dp > d_pos:
                worst = s
            d_pos, d_rot = max(d_pos, dp), max(d_rot, dr)
        # a count may differ by a point whose 3-sigma gate sits within rounding of its threshold; poses may not differ
        parity = {"n": n_chk, "compared_with": "poses of the last timed step, same slots, same map (device blob imported into the oracle)",
                  "counts_equal": cnt_eq, "max_pos_delta_m": d_pos, "max_rot_delta": d_rot, "tolerance_m": 1e-7,
                  "ok": bool(d_pos <= 1e-7 and d_rot <= 1e-7 and cnt_eq >= n_chk - max(1, n_chk // 50)), "worst_slot": worst}
        if c2 is not None:   # config 2: the oracle's residual build (KILO.cc:122-210) on the same scans under the same states, rows compared
            h6d, zd, Rd, vd = c2
            n_c2 = len(vd) // N_PTS
            t2s, c2_flips, c2_dh, c2_dz, c2_dR, c2_ok = [], 0, 0.0, 0.0, 0.0, True
            for s in range(n_c2):
                a_, b_ = s * N_PTS, (s + 1) * N_PTS
                xb_ = xyz_of(scans[tile[s]])
                o.set_state(xs[s], Ps[s])
                tc = time.perf_counter()
                ho, zo, Ro, vo = o.residuals(xb_)
                t2s.append(time.perf_counter() - tc)
                c2_flips += int((vo != vd[a_:b_]).sum())
                m = (vo & vd[a_:b_]).astype(bool)
                sg = np.sign(np.sum(h6d[a_:b_][m, 3:] * ho[m, 3:], axis=1))     # rows are defined up to the sign of the plane normal
                c2_dh = max(c2_dh, float(np.abs(h6d[a_:b_][m] - ho[m] * sg[:, None]).max()))
                c2_dz = max(c2_dz, float(np.abs(zd[a_:b_][m] - zo[m] * sg).max()))
                c2_dR = max(c2_dR, float(np.abs(Rd[a_:b_][m] / Ro[m] - 1.0).max()))
            # the allowance of test_config2_full_size_residuals: a point whose 3-sigma gate sits within rounding of its threshold may flip
            c2_ok = bool(c2_flips <= n_c2 and c2_dh <= 1e-8 and c2_dz <= 1e-7 and c2_dR <= 1e-7)
            parity["config2_rows"] = {"n_scans": n_c2, "points": n_c2 * N_PTS, "valid_mask_flips": c2_flips, "max_abs_dh": c2_dh, "max_abs_dz": c2_dz,
                                      "max_rel_dR": c2_dR, "ok": c2_ok, "checker": "oracle.residuals (KILO.cc:122-210) per scan on the device's map blob, same state"}
            parity["ok"] = bool(parity["ok"] and c2_ok)
            extra["config2_cpu_port_scans_per_s"] = round(1.0 / float(np.median(t2s)), 2)
            extra["config2_cpu_port_ns_per_point"] = round(float(np.median(t2s)) * 1e9 / N_PTS, 1)
            extra["config2_speedup_vs_cpu_port"] = round(extra["config2_scans_per_s"] / extra["config2_cpu_port_scans_per_s"], 1)
        if c1 is not None:   # the same config-1 scans on the CPU port, one at a time (frozen map), and the same comparison
            c1_scans_, c1_tb_, xs1, Ps1, tile1, p1, p1ov = c1
            t1s, c1_dpos, c1_eq = [], 0.0, 0
            for s in range(min(16, len(tile1))):
                u = tile1[s]
                o.set_state(xs1[s], Ps1[s].reshape(30, 30))
                o.set_times(c1_tb_[u], c1_tb_[u])
                tc = time.perf_counter()
                pose, _ = o.process_scan(c1_scans_[u], c1_tb_[u], with_sort=True)
                t1s.append(time.perf_counter() - tc)
                c1_dpos = max(c1_dpos, float(np.abs(np.array(pose.pos) - p1[s]["pos"]).max()))
                c1_eq += int((int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect)) == (int(p1[s]["n_buckets"]), int(p1[s]["n_updates"]), int(p1[s]["n_effect"])))
            extra["config1_cpu_port_scans_per_s"] = round(1.0 / float(np.median(t1s)), 1)
            extra["config1_speedup_vs_cpu_port"] = round(extra["config1_ragged_scans_per_s"] / extra["config1_cpu_port_scans_per_s"], 1)
            parity["config1_ragged"] = {"n": len(t1s), "counts_equal": c1_eq, "max_pos_delta_m": c1_dpos}
            parity["ok"] = bool(parity["ok"] and c1_dpos <= 1e-7)
            if p1ov is not None:   # the recorded-run batch WITH insert: the oracle with insert ON on a private copy of the map, scan by scan
                o_eq, o_dpos, t1o = 0, 0.0, []
                n_o = min(8, len(p1ov))
                for s in range(n_o):
                    u = tile1[s]
                    o.map_import(map_blob_for_oracle)
                    o.set_map_insert(True)
                    o.set_state(xs1[s], Ps1[s].reshape(30, 30))
                    o.set_times(c1_tb_[u], c1_tb_[u])
                    tc = time.perf_counter()
                    pose, _ = o.process_scan(c1_scans_[u], c1_tb_[u], with_sort=True)
                    t1o.append(time.perf_counter() - tc)
                    o_dpos = max(o_dpos, float(np.abs(np.array(pose.pos) - p1ov[s]["pos"]).max()))
                    o_eq += int((int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect)) == (int(p1ov[s]["n_buckets"]), int(p1ov[s]["n_updates"]), int(p1ov[s]["n_effect"])))
                o.map_import(map_blob_for_oracle)
                o.set_map_insert(False)
                parity["config1_overlay_ragged"] = {"n": n_o, "counts_equal": o_eq, "max_pos_delta_m": o_dpos, "tolerance_m": 1e-7}
                parity["ok"] = bool(parity["ok"] and o_dpos <= 1e-7 and o_eq >= n_o - 1)
                extra["config1_overlay_cpu_port_scans_per_s"] = round(1.0 / float(np.median(t1o)), 1)
        if c4 is not None:   # config 4: the same run on the CPU port (kinematic + IMU mode, insert on) and on the reference's own build
            cfg4, x04, xw4, xb4, ds4, tb4, kins4, poses4 = c4
            runs4 = [("port", lambda: ob.Oracle(cfg4, imu_mode_only=False))]
            if ob.build_ref() is not None:
                import tempfile

                yml4 = os.path.join(tempfile.mkdtemp(prefix="lkc4"), "c4.yaml")
                runs4.append(("reference", lambda: ob.ReferenceKilo(config.DITER, False, yml4)))
            c4par = {}
            for name, mk in runs4:
                r4 = mk()
                r4.set_state(x04, 1e-6 * np.eye(30))
                r4.init_process_cov_q()
                r4.set_acc_norm(9.81)
                r4.set_times(T0_CONFIG4, T0_CONFIG4)
                r4.map_build(xw4, xb4)
                t4s, eq4, dpos4 = [], 0, 0.0
                for k in range(len(ds4)):
                    tc = time.perf_counter()
                    pose, _ = r4.process_scan(ds4[k], tb4[k], kins=kins4[k], with_sort=True)
                    t4s.append(time.perf_counter() - tc)
                    nb_, nu_, ne_, pos_, _ = poses4[k]
                    eq4 += int(int(pose.n_effect) == ne_ and (name != "port" or (int(pose.n_buckets), int(pose.n_updates)) == (nb_, nu_)))
                    dpos4 = max(dpos4, float(np.abs(np.array(pose.pos) - pos_).max()))
                r4.close()
                c4par[name] = {"n": len(ds4), "counts_equal": eq4, "max_pos_delta_m": dpos4}
                extra[f"config4_cpu_{name}_ms_per_scan"] = round(float(np.median(t4s[1:])) * 1e3, 3)
                extra[f"config4_path_speedup_vs_cpu_{name}"] = round(float(np.median(t4s[1:])) * 1e3 / extra["config4_path_ms_per_scan"], 2)
            # closed loop with insert over 100 scans: counts are exact, positions agree to the closed-loop sensitivity of DESIGN section 7 (1e-6 m)
            parity["config4_live"] = dict(c4par, tolerance_m=1e-6, checker="oracle / oracle/_ref KILO::process, leg fusion, insert on, same messages and scans")
            parity["ok"] = bool(parity["ok"] and all(v["counts_equal"] == v["n"] and v["max_pos_delta_m"] <= 1e-6 for v in c4par.values()))
        if shuf is not None:   # the shuffled batch's own parity sample: same oracle, same map, the scans as the device got them (the sort is stable)
            sh_host, sh_last = shuf
            sh_eq, sh_dpos = 0, 0.0
            for s_ in range(len(sh_host)):
                o.set_state(xs[s_], Ps[s_])
                o.set_times(0.0, 0.0)
                pose, _ = o.process_scan(sh_host[s_], 0.0, with_sort=True)
                sl_ = sh_last[s_]
                sh_eq += int((int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect)) == (int(sl_["n_buckets"]), int(sl_["n_updates"]), int(sl_["n_effect"])))
                sh_dpos = max(sh_dpos, float(np.abs(np.array(pose.pos) - sl_["pos"]).max()))
            parity["shuffled_in_bucket"] = {"n": len(sh_host), "counts_equal": sh_eq, "max_pos_delta_m": sh_dpos, "tolerance_m": 1e-7}
            parity["ok"] = bool(parity["ok"] and sh_dpos <= 1e-7 and sh_eq >= len(sh_host) - max(1, len(sh_host) // 50))
        if shuf_auto is not None:   # the shuffled buffer replayed from the library's own voxel-ordered copy: the oracle on the scans as the CALLER gave them
            sh_host, au_last = shuf_auto
            au_eq, au_dpos = 0, 0.0
            for s_ in range(min(len(sh_host), 8)):
                o.set_state(xs[s_], Ps[s_])
                o.set_times(0.0, 0.0)
                pose, _ = o.process_scan(sh_host[s_], 0.0, with_sort=True)
                sl_ = au_last[s_]
                au_eq += int((int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect)) == (int(sl_["n_buckets"]), int(sl_["n_updates"]), int(sl_["n_effect"])))
                au_dpos = max(au_dpos, float(np.abs(np.array(pose.pos) - sl_["pos"]).max()))
            parity["shuffled_auto"] = {"n": min(len(sh_host), 8), "counts_equal": au_eq, "max_pos_delta_m": au_dpos, "tolerance_m": 1e-7}
            parity["ok"] = bool(parity["ok"] and au_dpos <= 1e-7 and au_eq >= min(len(sh_host), 8) - 1)
        if resorted is not None:   # the device-sorted batch: the oracle replays the scans as lk_batch_sort_by_voxel_dev left them
            rs_host, rs_last = resorted
            rs_eq, rs_dpos = 0, 0.0
            for s_ in range(len(rs_host)):
                o.set_state(xs[s_], Ps[s_])
                o.set_times(0.0, 0.0)
                pose, _ = o.process_scan(rs_host[s_], 0.0, with_sort=True)
                sl_ = rs_last[s_]
                rs_eq += int((int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect)) == (int(sl_["n_buckets"]), int(sl_["n_updates"]), int(sl_["n_effect"])))
                rs_dpos = max(rs_dpos, float(np.abs(np.array(pose.pos) - sl_["pos"]).max()))
            parity["shuffled_resorted"] = {"n": len(rs_host), "counts_equal": rs_eq, "max_pos_delta_m": rs_dpos, "tolerance_m": 1e-7}
            parity["ok"] = bool(parity["ok"] and rs_dpos <= 1e-7 and rs_eq >= len(rs_host) - 1)
        # and the full config-3 path with insert (the reference's own timed lambda, KILO.cc:367-396)
        o.set_map_insert(True)
        o.set_state(synth.initial_state(traj, t_after, P), 1e-6 * np.eye(30))
        o.set_times(t_after, t_after)
        tfull = []
        n_full = min(len(sscans), max(3, args.cpu_sample // 6))   # consecutive scans: the map keeps growing as in a run
        for k in range(n_full):
            tc = time.perf_counter()
            o.process_scan(sscans[k], t_after + 0.1 * k, with_sort=True)
            tfull.append(time.perf_counter() - tc)
        if ov is not None and args.overlay_check > 0:
            # the overlay replay against the oracle: each scan on a PRIVATE copy of the device's map (blob re-imported), insert on
            n_oc = min(args.overlay_check, len(ov))
            oc_eq, oc_dpos, oc_t = 0, 0.0, []
            for s in range(n_oc):
                o.map_import(map_blob_for_oracle)
                o.set_map_insert(True)
                o.set_state(xs[s], Ps[s])
                o.set_times(0.0, 0.0)
                tc = time.perf_counter()
                pose, _ = o.process_scan(scans[tile[s]], 0.0, with_sort=True)
                oc_t.append(time.perf_counter() - tc)
                oc_eq += int((int(pose.n_buckets), int(pose.n_updates), int(pose.n_effect)) == (int(ov[s]["n_buckets"]), int(ov[s]["n_updates"]), int(ov[s]["n_effect"])))
                oc_dpos = max(oc_dpos, float(np.abs(np.array(pose.pos) - ov[s]["pos"]).max()))
            parity["overlay"] = {"n": n_oc, "counts_equal": oc_eq, "max_pos_delta_m": oc_dpos, "tolerance_m": 1e-7,
                                 "checker": "oracle.process_scan with insert ON on a private copy of the device's map blob"}
            parity["ok"] = bool(parity["ok"] and oc_dpos <= 1e-7 and oc_eq >= n_oc - max(1, n_oc // 50))
            extra["overlay_cpu_port_scans_per_s"] = round(1.0 / float(np.median(oc_t)), 2)
            extra["overlay_speedup_vs_cpu_port"] = round(extra["overlay_scans_per_s"] / extra["overlay_cpu_port_scans_per_s"], 1)
        o.close()
        cpu_baseline = {
            "value": round(1.0 / float(np.median(tcs)), 3), "unit": "scans/s", "cores": 1, "kind": "port",
            "sample": f"{n_chk} of the batch's 100k-pt scans (5 buckets, frozen map = the device's map blob, 6x6-form update), "
                      f"{sum(tcs):.1f} s of CPU time, median per scan, sort included (KILO.cc:367-396); full path with insert: "
                      f"{len(tfull)} consecutive scans, {sum(tfull):.1f} s",
            "full_path_with_insert_scans_per_s": round(1.0 / float(np.median(tfull)), 3) if tfull else None,
            "host_cores_available": os.cpu_count(),
        }
        # ---- for the record: the REFERENCE's own build (oracle/_ref: KILO.cc / eskf.cc / voxel_map.cc compiled unmodified, literal
        # N x N updateByPoints, eskf.cc:105-112) on the config-1 scans, and the literal form extrapolated to 20 000-point buckets
        cpu_baseline["reference_literal"] = reference_literal(ob, cfg, P, traj, c1, map_blob_for_oracle, tcs)
        extra["speedup_vs_cpu_port"] = round(value / cpu_baseline["value"], 1)
        if "stream_scans_per_s" in extra and tfull:
            extra["stream_speedup_vs_cpu_port"] = round(extra["stream_scans_per_s"] / cpu_baseline["full_path_with_insert_scans_per_s"], 1)

    if rank == 0:
        wl = (f"config5: batch replay of {S if not strong else args.total_scans} synthetic 100k-pt scans "
              f"{'per GPU' if not strong else 'in total, block-sharded over the GPUs'}, {U} distinct scans per GPU"
              f"{'' if U == S else f' TILED x{S // U} to the batch (priors still distinct)'}, every scan at its own pose with its own prior, "
              "5 buckets x 20k, full ESKF update, shared frozen voxel map built from 20 warm-up scans over the trajectory (RCCL broadcast when N>1)")
        line = {
            "metric": "LiDAR scans/sec (per-point ESKF update), 100k-pt scan", "value": round(value, 2), "unit": "scans/s",
            "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": wl, "scans_per_gpu": S, "unique_scans_per_gpu": U, "total_scans": args.total_scans if strong else S * world_size,
                       "points_per_scan": N_PTS, "buckets": N_BUCKETS, "parallelism": f"replay-shard x{world_size}"},
            "roofline": roofline, "cpu_baseline": cpu_baseline, "parity_check": parity, "extra": extra,
        }
        if warnings:
            line["warnings"] = warnings
        print(json.dumps(line))
    g.close()
    if dist is not None:
        dist.destroy_process_group()
    if parity is not None and not parity["ok"]:
        sys.stderr.write(f"bench.py: PARITY VIOLATION between the timed loop and the oracle: {parity}\n")
        sys.exit(3)


def reference_literal(ob, cfg, P, traj, c1, blob, tcs_port):
    """Time the reference's own KILO::process (oracle/_ref) where it can run: the config-1 scans (buckets of tens of points,
    literal N x N inverse) on its own map; extrapolate the literal update to this bench's 20 000-point buckets."""
    out = {"available": False}
    try:
        if c1 is None or ob.build_ref() is None:
            out["why"] = "oracle/_ref not built on this box or config-1 extra disabled"
            return out
        import tempfile

        c1_scans, c1_tb = c1[0], c1[1]
        yml = os.path.join(tempfile.mkdtemp(prefix="lkref"), "ref.yaml")
        world = synth.World()
        t00 = c1_tb[0] - 0.1
        x0 = synth.initial_state(traj, t00, P)
        raw = synth.vlp16_scan(world, Frozen(traj, t00), t00, P)
        xb = xyz_of(raw)
        res = {}
        # the reference's own process() needs the scan's IMU packet (KILO.cc:326): the real config-1 mode, IMU updates between the
        # buckets (only_imu_use); the port runs the identical call sequence beside it
        for name, mk in (("reference", lambda: ob.ReferenceKilo(P, True, yml)), ("port", lambda: ob.Oracle(cfg, imu_mode_only=True))):
            r = mk()
            r.set_state(x0, 1e-6 * np.eye(30))
            r.init_process_cov_q()
            r.set_acc_norm(9.81)
            r.set_times(t00, t00)
            r.map_build(world_of(x0, xb, P), xb)
            ts, neff = [], []
            for k in range(len(c1_scans)):
                imus = synth.imu_stream(traj, c1_tb[k], c1_tb[k] + 0.1, seed=3003 + k)
                r.set_state(synth.initial_state(traj, c1_tb[k], P), 1e-6 * np.eye(30))
                r.set_times(c1_tb[k], c1_tb[k])
                tc = time.perf_counter()
                pose, _ = r.process_scan(c1_scans[k], c1_tb[k], imus=imus, with_sort=True)
                ts.append(time.perf_counter() - tc)
                neff.append(int(pose.n_effect))
            r.close()
            res[name] = (ts, neff)
        ts, neff = res["reference"]
        if min(neff) <= 0:
            out["why"] = "the reference build did not process the scans (n_effect = 0)"
            return out
        # literal-form cost model: the N x N inverse dominates, ~ (2/3 + 2) N^3 flop for LU + solve against I; calibrate the
        # per-flop time on a dense N = 600 inverse with numpy (LAPACK, one thread is what Eigen's would be at best)
        Ncal = 600
        A = np.random.default_rng(1).normal(size=(Ncal, Ncal)) + Ncal * np.eye(Ncal)
        tc = time.perf_counter()
        np.linalg.inv(A)
        t_inv = time.perf_counter() - tc
        per_flop = t_inv / (2.0 * Ncal ** 3)
        Nb = 0.6 * (N_PTS // N_BUCKETS)      # ~60 % of a 20 000-point bucket matches
        lit_s = N_BUCKETS * 2.0 * Nb ** 3 * per_flop
        out = {
            "available": True, "what": "oracle/_ref = the reference's KILO.cc/eskf.cc/voxel_map.cc compiled unmodified (mini-Eigen stand-in: "
                                       "naive dense kernels, so this is an upper bound on the reference's time, not its best)",
            "config1_scans_per_s": round(1.0 / float(np.median(ts)), 2), "config1_scans": len(ts), "config1_mean_n_effect": float(np.mean(neff)),
            "config1_port_same_calls_scans_per_s": round(1.0 / float(np.median(res["port"][0])), 2),
            "config1_counts_equal_reference_vs_port": bool(neff == res["port"][1]),
            "literal_100k_extrapolated_s_per_scan": round(lit_s, 1),
            "literal_100k_extrapolation": f"5 buckets x 2 N^3 flop at N = {int(Nb)} matched rows, {per_flop * 1e12:.2f} ps/flop from a LAPACK "
                                          f"{Ncal} x {Ncal} inverse on this host; memory N^2 x 8 B = {Nb * Nb * 8 / 1e9:.1f} GB per bucket",
            "port_100k_s_per_scan": round(float(np.median(tcs_port)), 4),
        }
        lit51 = os.path.join(ROOT, "profiles", "r05_cpu_literal_51.json")
        if os.path.exists(lit51):   # BASELINE.md section 2 figure (i), MEASURED once (tools/cpu_literal_51.py: minutes per scan), quoted here
            j = json.load(open(lit51))
            out["literal_51_buckets_s_per_scan_measured"] = j.get("literal_51_buckets_s_per_scan_measured")
            out["literal_51_buckets_measured_on"] = f"{j.get('cpu_model')}, {j.get('cores_used')} core, oracle port with literal_max_n raised (profiles/r05_cpu_literal_51.json)"
            out["info6_51_buckets_s_per_scan_same_scan"] = j.get("info6_51_buckets_s_per_scan_measured")
    except Exception as e:  # noqa: BLE001
        out["error"] = f"{type(e).__name__}: {str(e)[:200]}"
    return out


if __name__ == "__main__":
    main()
