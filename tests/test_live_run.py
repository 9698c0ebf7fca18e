"""lk_run_scans_dev: a recorded run LIVE on slot 0, in one call, from device-resident scans and message records.

The reference of every GPU test is a SECOND handle driven by a Python loop of process_scan over host copies of the same scans and messages
(bit for bit: the entry runs the same kernels in the same order, chosen per scan from device-side summaries of device-built bucket tables),
and, where stated, the CPU oracle.  The entry under test is never its own reference."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import devguard
import scenes
from legkilo_amd import abi, config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
PT, IMU_REC, KIN_REC = synth.POINT_DTYPE.itemsize, synth.IMU_DTYPE.itemsize, synth.KIN_DTYPE.itemsize
T0 = 21.0


# ------------------------------------------------------------------ shared inputs and helpers
@functools.lru_cache(maxsize=None)
def _scene(kind):
    """msg_kind 2 runs on diter.yaml's parameters like test_sequence_kin_mode, the others on the default scene."""
    return scenes.Scene(params=config.DITER, **CAPS) if kind == 2 else scenes.Scene(**CAPS)


@functools.lru_cache(maxsize=None)
def _config1_run(kind, sc=None):
    """4 config-1 scans (hundreds of small buckets each) with their messages: generated once, shared, never modified.
    sc: a ready scene (tests/placement.py) instead of _scene(kind)."""
    sc = sc or _scene(kind)
    scans, tbs, msgs = [], [], []
    for k in range(4):
        tb = T0 + 0.1 * k
        scans.append(scenes.vlp_scan_input(sc, tb, k))
        tbs.append(tb)
        if kind == 2:
            msgs.append(synth.kin_stream(sc.traj, tb, tb + 0.1, sc.P, seed=3003 + k))
        elif kind == 1:
            msgs.append(synth.imu_stream(sc.traj, tb, tb + 0.1, seed=3003 + k))
    for a in scans + msgs:
        a.setflags(write=False)
    return scans, tbs, (msgs if kind else None)


def _start(obj, sc, t0=T0):
    x0 = scenes.init_filter(obj, sc, t0)
    scenes.first_frame(obj, sc, t0, x0)


def _msg_kw(kind, msgs):
    return {} if not kind else ({"imus": msgs} if kind == 1 else {"kins": msgs})


def _loop(g, scans, tbs, kind, msgs, slide=None):
    """The parent path: process_scan scan by scan over host copies (+ map_slide behind every scan) -> (poses, worlds, slid flags)."""
    poses, worlds, slid = [], [], []
    for s, (pts, tb) in enumerate(zip(scans, tbs)):
        kw = _msg_kw(kind, msgs[s] if kind else None)
        kw = {k: (v if len(v) else None) for k, v in kw.items()}
        pose, w = g.process_scan(pts, tb, want_world=True, **kw)
        poses.append(pose), worlds.append(w)
        if slide is not None:
            slid.append(g.map_slide(np.array(pose.pos), *slide))   # (slid, roots removed)
    return poses, worlds, slid


def _same_pose(a, b, where):
    for f, _ in abi.lk_pose._fields_:
        va, vb = getattr(a, f), getattr(b, f)
        assert (list(va) == list(vb)) if hasattr(va, "__len__") else (va == vb), (where, f)


def _digest(g):
    x, P = g.get_state()
    return x.tobytes(), P.tobytes(), g.get_times(), g.map_export()


def _same_handle_state(g, g_ref):
    (xa, Pa, ta, ma), (xb, Pb, tb, mb) = _digest(g), _digest(g_ref)
    assert xa == xb, "x36 differs"
    assert Pa == Pb, "P900 differs"
    assert ta == tb, ("time stamps differ", ta, tb)
    return scenes.maps_identical(ma, mb)


def _close(*objs):
    for o in objs:
        o.close()


# ------------------------------------------------------------------ 1. bit identity with the per-scan loop
@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_run_equals_the_per_scan_loop(hip_lib, kind):
    sc = _scene(kind)
    scans, tbs, msgs = _config1_run(kind)
    g_loop, g_run, g_now = (hip_lib.LegKiloHip(sc.cfg()) for _ in range(3))
    for g in (g_loop, g_run, g_now):
        _start(g, sc)
    ref_poses, ref_worlds, _ = _loop(g_loop, scans, tbs, kind, msgs)
    assert min(p.n_buckets for p in ref_poses) > 100 and min(int(p.n_effect) for p in ref_poses) > 0
    poses, worlds, n_slides = g_run.run_scans(scans, tbs, world=True, **_msg_kw(kind, msgs))
    assert len(poses) == 4 and n_slides == 0
    for s in range(4):
        _same_pose(poses[s], ref_poses[s], s)
        assert np.array_equal(worlds[s], ref_worlds[s]), s
    assert _same_handle_state(g_run, g_loop) > 100
    # d_world_out NULL: the same state
    poses2, worlds2, _ = g_now.run_scans(scans, tbs, world=False, **_msg_kw(kind, msgs))
    assert worlds2 is None
    for s in range(4):
        _same_pose(poses2[s], ref_poses[s], s)
    _same_handle_state(g_now, g_loop)
    assert g_run.stream_resident_stats() == g_loop.stream_resident_stats() and g_run.stream_resident_stats()[0] == 4
    _close(g_loop, g_run, g_now)


# ------------------------------------------------------------------ 2. against the oracle
@pytest.mark.gpu
def test_run_against_the_oracle(oracle_lib, hip_lib):
    """The msg_kind 1 run of test 1 through the oracle's KILO::process replay: counts exact per scan, positions to the tolerance of
    test_sequence_imu_mode[literal=False] (the oracle's 6 x 6 form: only the summation order differs): 1e-7 m, per scan and as ATE."""
    sc = _scene(1)
    scans, tbs, msgs = _config1_run(1)
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    o.set_literal_max_n(0)
    g = hip_lib.LegKiloHip(sc.cfg())
    for obj in (o, g):
        _start(obj, sc)
    ref = [o.process_scan(scans[s], tbs[s], imus=msgs[s])[0] for s in range(4)]
    ref_pos = [np.array(p.pos) for p in ref]
    poses, _, _ = g.run_scans(scans, tbs, imus=msgs)
    tol, worst = 1e-7, 0.0
    for s in range(4):
        assert (ref[s].n_buckets, ref[s].n_updates, ref[s].n_effect) == (poses[s].n_buckets, poses[s].n_updates, poses[s].n_effect), s
        worst = max(worst, np.abs(ref_pos[s] - np.array(poses[s].pos)).max())
    ate = scenes.ate(ref_pos, [np.array(p.pos) for p in poses])
    print(f"one-call run vs oracle: worst position delta {worst:.3e} m, ATE delta {ate:.3e} m")
    assert worst < tol, worst
    assert ate < tol, ate
    xo, xg = o.get_state()[0], g.get_state()[0]
    assert np.abs(xo[9:12] - xg[9:12]).max() < tol
    scenes.compare_maps(o.map_export(), g.map_export(), rtol=1e-5, ptol=10 * tol)
    _close(g, o)


# ------------------------------------------------------------------ 3. kernel choice per scan from the device summaries
def _shaped_scan(sc, tb, sizes, seed, dcurv=0.002):
    """A hand-made scan: bucket k holds sizes[k] points at curvature dcurv * (k + 1)."""
    pts = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=sum(sizes), n_buckets=1, seed_scan=seed, seed_noise=seed + 100).copy()
    pts["curvature"] = np.concatenate([np.full(n, np.float32(dcurv * (k + 1))) for k, n in enumerate(sizes)])
    return pts


@functools.lru_cache(maxsize=None)
def _mixed_run():
    sc = _scene(1)
    shapes = [[40, 64, 17, 1, 50, 33], [600, 600, 600], [600], [9, 64, 2, 31]]
    scans = [_shaped_scan(sc, T0 + 0.1 * k, sz, 7300 + k) for k, sz in enumerate(shapes)]
    tbs = [T0 + 0.1 * k for k in range(4)]
    # messages from 4 ms before the scan on: some stamped before the first bucket, some between buckets, most after the last one (left unused)
    imus = [synth.imu_stream(sc.traj, tb - 0.004, tb + 0.02, seed=5003 + k) for k, tb in enumerate(tbs)]
    imus[1] = imus[1][:0]   # three buckets of 600 points, no messages: the grid-resident kernel's scan
    assert (imus[2]["stamp"] < tbs[2] + 0.002).sum() > 0   # the 600-point bucket has messages in front of it
    return scans, tbs, imus


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "resident-off", "grid-off"])
def test_kernel_choice_per_scan(hip_lib, mode):
    """Small buckets | 3 x 600 points without messages | 1 x 600 points with IMU messages | small buckets: scan-resident, grid-resident (or
    per-bucket launches), per-bucket launches with messages, scan-resident - the same choices on both handles, read off the statistics."""
    sc = _scene(1)
    scans, tbs, imus = _mixed_run()
    g_loop, g_run = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    for g in (g_loop, g_run):
        _start(g, sc)
        if mode == "resident-off":
            g.stream_resident(False)
        if mode == "grid-off":
            g.stream_grid(0)
    before = [(g.stream_resident_stats(), g.stream_stats()) for g in (g_loop, g_run)]
    ref_poses, ref_worlds, _ = _loop(g_loop, scans, tbs, 1, imus)
    assert [p.n_buckets for p in ref_poses] == [6, 3, 1, 4]
    poses, worlds, _ = g_run.run_scans(scans, tbs, imus=imus, world=True)
    for s in range(4):
        _same_pose(poses[s], ref_poses[s], s)
        assert np.array_equal(worlds[s], ref_worlds[s]), s
    _same_handle_state(g_run, g_loop)
    after = [(g.stream_resident_stats(), g.stream_stats()) for g in (g_loop, g_run)]
    moved = [tuple(int(v) for v in np.r_[np.subtract(a[0], b[0]), np.subtract(a[1], b[1])]) for a, b in zip(after, before)]
    print(f"{mode}: resident / stream statistics moved by {moved[0]} (loop) {moved[1]} (one call)")
    assert moved[0] == moved[1], moved
    # scans through a resident kernel: the two small-bucket scans (scan-resident) and the 3 x 600 scan (grid-resident)
    assert moved[0][0] == {"default": 3, "resident-off": 1, "grid-off": 2}[mode], moved
    _close(g_loop, g_run)


# ------------------------------------------------------------------ 3b. lk_process_scan_dev: a hand-written table against process_scan
# bucket sizes, 0 = an empty table entry: scan-resident with empty entries first, inside and last | grid-resident | an empty entry between two
# large buckets | mixed sizes (per-bucket launches) | one large bucket
PSD_SHAPES = [[0, 1, 64, 0, 65, 512, 0], [513, 600, 513], [513, 0, 600], [40, 513, 9], [513]]


def _hand_table(sizes, dcurv=0.002):
    """(bucket_off, bucket_dt) of _shaped_scan(sizes): entry k holds sizes[k] points at the float32 curvature dcurv * (k + 1); an empty entry
    repeats its neighbour's time (the one before it, or the one behind it where it is first)."""
    dt = [float(np.float32(dcurv * (k + 1))) if n else None for k, n in enumerate(sizes)]
    first = next((v for v in dt if v is not None), 0.0)
    for k in range(len(dt)):
        if dt[k] is None:
            dt[k] = dt[k - 1] if k else first
    return np.r_[0, np.cumsum(sizes)].astype(np.uint32), np.array(dt)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "resident-off", "grid-off"])
def test_process_scan_dev_equals_process_scan(hip_lib, mode):
    """Handle A: process_scan over the host copy of a scan (its buckets found from the curvatures).  Handle B: the same points in HBM and
    process_scan_dev with a hand-written bucket table that also holds empty entries.  Same pose, same filter, same map, same kernel choice,
    scan after scan; then a table of empty entries only: a pose with n_buckets == 0, filter and map untouched."""
    sc = _scene(1)
    g_a, g_b = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    for g in (g_a, g_b):
        _start(g, sc)
        if mode == "resident-off":
            g.stream_resident(False)
        if mode == "grid-off":
            g.stream_grid(0)
    d_pts = g_b.device_malloc(max(sum(sz) for sz in PSD_SHAPES) * PT)
    try:
        for k, sizes in enumerate(PSD_SHAPES):
            tb = T0 + 0.1 * k
            pts = _shaped_scan(sc, tb, sizes, 7700 + k)
            off, dt = _hand_table(sizes)
            before = [g.stream_resident_stats() for g in (g_a, g_b)]
            pose_a, _ = g_a.process_scan(pts, tb)
            g_b.h2d(d_pts, pts)
            pose_b = g_b.process_scan_dev(d_pts, len(pts), tb, off, dt)
            assert pose_a.n_buckets == sum(1 for n in sizes if n), (sizes, pose_a.n_buckets)
            _same_pose(pose_b, pose_a, sizes)
            _same_handle_state(g_b, g_a)
            moved = [tuple(int(v) for v in np.subtract(g.stream_resident_stats(), b)) for g, b in zip((g_a, g_b), before)]
            print(f"{mode} {sizes}: resident statistics moved by {moved[0]} (process_scan) {moved[1]} (process_scan_dev)")
            assert moved[0] == moved[1], (sizes, moved)
        # empty entries only (over a scan that has points: n == 0 is refused)
        state, stats = _digest(g_b), g_b.stream_resident_stats()
        pose = g_b.process_scan_dev(d_pts, len(pts), T0 + 0.1 * len(PSD_SHAPES), np.zeros(3, dtype=np.uint32), np.zeros(2))
        assert pose.n_buckets == 0
        after = _digest(g_b)
        assert after[:2] == state[:2], "state changed"
        scenes.maps_identical(after[3], state[3])
        assert g_b.stream_resident_stats() == stats
    finally:
        g_b.device_free(d_pts)
        _close(g_a, g_b)


# ------------------------------------------------------------------ 4. edge sizes, sub-range, guard bands
@pytest.mark.gpu
def test_edge_sizes_and_subrange_with_guard_bands(hip_lib):
    """Scans of 1, 63, 64, 65 and 257 points, first as ONE bucket each, then as one point per bucket; scan_off[0] != 0 with a poisoned scan in
    front of it (NaN coordinates, decreasing non-finite curvature: reading it would refuse the run or poison the filter); d_pts, d_msgs and
    d_world_out inside guard bands; scans without messages; messages stamped after a scan's last bucket."""
    sc = _scene(1)
    sizes = [1, 63, 64, 65, 257]
    scans, tbs = [], []
    for k, n in enumerate(sizes + sizes):
        tb = T0 + 0.1 * k
        scans.append(_shaped_scan(sc, tb, [n] if k < 5 else [1] * n, 7600 + k, dcurv=0.0002))
        tbs.append(tb)
    imus = [synth.imu_stream(sc.traj, tb - 0.004, tb + 0.07, seed=5103 + k) for k, tb in enumerate(tbs)]
    for k in (0, 3, 7):
        imus[k] = imus[k][:0]
    assert all(len(im) == 0 or im["stamp"][-1] > tb + 0.06 for im, tb in zip(imus, tbs))   # stamped after the last bucket: left unused (KILO.cc:379-390)
    poison = np.zeros(100, dtype=synth.POINT_DTYPE)
    poison["x"] = poison["y"] = poison["z"] = np.nan
    poison["curvature"] = np.r_[np.linspace(1.0, 0.0, 98), np.nan, -np.inf].astype(np.float32)
    allpts = np.concatenate([poison] + scans)
    scan_off = (len(poison) + np.r_[0, np.cumsum([len(s) for s in scans])]).astype(np.uint64)
    n_msg = np.array([len(im) for im in imus], dtype=np.uint32)
    flat = np.concatenate([im for im in imus if len(im)])

    g_loop, g_run = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    for g in (g_loop, g_run):
        _start(g, sc)
    ref_poses, ref_worlds, _ = _loop(g_loop, scans, tbs, 1, imus)
    assert [p.n_buckets for p in ref_poses] == [1] * 5 + sizes
    bufs = []
    try:
        d_pts = devguard.Guarded.input(g_run, allpts, offset=16, name="run d_pts")
        d_msgs = devguard.Guarded.input(g_run, flat, offset=8, name="run d_msgs")
        d_world = devguard.Guarded(g_run, 16 * len(allpts), offset=16, name="run d_world_out")
        bufs = [d_pts, d_msgs, d_world]
        poses, n_slides = g_run.run_scans_dev(d_pts.ptr, scan_off, tbs, 1, n_msg, d_msgs.ptr, None, d_world.ptr)
        d_pts.check(), d_msgs.check()
        w = d_world.read(np.float32).reshape(-1, 4)
        devguard.untouched(w[: len(poison)].view(np.uint8))   # nothing in front of scan_off[0] is written either
        got = w[len(poison):]
        devguard.sentinel_free(got)
        for s in range(len(scans)):
            _same_pose(poses[s], ref_poses[s], s)
            a, b = int(scan_off[s]) - len(poison), int(scan_off[s + 1]) - len(poison)
            assert np.array_equal(got[a:b, :3], ref_worlds[s]), s
        _same_handle_state(g_run, g_loop)
    finally:
        for b in bufs:
            b.free()
        _close(g_loop, g_run)


# ------------------------------------------------------------------ 5. sliding
@pytest.mark.gpu
def test_run_with_map_sliding(hip_lib):
    run_with_map_sliding(hip_lib)


def run_with_map_sliding(hip_lib, sc=None):
    scans, tbs, msgs = _config1_run(1) if sc is None else _config1_run(1, sc)
    sc = sc or _scene(1)
    slide = (0.05, 12)   # metres moved since the last slide; half box size in voxels: far voxels of the first frame are dropped
    g_loop, g_run = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    for g in (g_loop, g_run):
        _start(g, sc)
    ref_poses, _, slid = _loop(g_loop, scans, tbs, 1, msgs, slide=slide)
    assert sum(f for f, _ in slid) >= 1, slid        # the loop's own flags first
    assert sum(n for _, n in slid) > 0, slid         # (and a slide dropped voxels: the maps below are equal because both slid)
    poses, _, n_slides = g_run.run_scans(scans, tbs, imus=msgs, slide=slide)
    assert n_slides == sum(f for f, _ in slid), (n_slides, slid)
    for s in range(4):
        _same_pose(poses[s], ref_poses[s], s)
    _same_handle_state(g_run, g_loop)
    assert np.array_equal(g_run.get_last_slide_position(), g_loop.get_last_slide_position())
    _close(g_loop, g_run)


# ------------------------------------------------------------------ 6. from message bytes
class _Standing:
    """A robot standing still at the trajectory's pose at t0 (the first frame takes gravity from the mean specific force)."""

    def __init__(self, tr, t0):
        self.tr, self.t0 = tr, t0

    def rot(self, tt):
        return self.tr.rot(np.full(np.shape(tt), self.t0))

    def pos(self, tt):
        return self.tr.pos(np.full(np.shape(tt), self.t0))

    def acc(self, tt):
        return np.zeros(np.shape(tt) + (3,))

    def omega_body(self, tt):
        return np.zeros(np.shape(tt) + (3,))


@pytest.mark.gpu
def test_run_from_message_bytes(hip_lib):
    """5 Velodyne PointCloud2 messages + Imu bytes -> lk_decode_scan_dev (raw first cloud) / lk_decode_scans_dev / lk_decode_imu_dev /
    lk_imu_split_dev -> lk_first_frame_dev on package 0, lk_run_scans_dev on packages 1 .. 4 straight from the front ends' device outputs
    (their tables shifted by one).  Equals, bit for bit, the same run done with read-backs: first_frame + the process_scan loop on a second
    handle fed with host copies of the decoded scans and records."""
    P = dict(config.LEG_FUSION, only_imu_use=True, redundancy=True, lidar_type=1, time_scale=1.0, filter_num=3, blind=1.5, voxel_grid_resolution=0.3)
    sc = scenes.Scene(params=P, **CAPS)
    t0, S = 2.0, 5
    still = _Standing(sc.traj, t0)
    stamps = [t0 + 0.1 * s for s in range(S)]
    msgs = [synth.cloud_message(synth.vlp16_scan(sc.world, still, tb, P, seed_noise=3083 + s), 1, tb, seed=s) for s, tb in enumerate(stamps)]
    buf, msg_off, n_points = synth.pack_cloud_run(msgs, seed=5)
    imus = synth.imu_stream(still, t0, stamps[-1] + 0.13, seed=8600)
    rng = np.random.default_rng(6)
    ibuf, ioff = synth.imu_messages(imus, [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(0, 41, len(imus))], seed=8)
    g, g_ref = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    dptrs = []
    try:
        g.imu_configure(P)
        total = int(n_points.sum())
        dptrs = [g.device_malloc(nb) for nb in (buf.nbytes, int(n_points[0]) * PT, total * PT, ibuf.nbytes, len(imus) * IMU_REC, total * 16)]
        d_bag, d_raw, d_pts, d_ibag, d_imus, d_world = dptrs
        g.h2d(d_bag, buf)
        g.h2d(d_ibag, ibuf)
        lay = synth.cloud_layout(1)
        n_raw, _, te0 = g.decode_scan_dev(d_bag + int(msg_off[0]), int(n_points[0]), lay, 1.0, P["filter_num"], P["blind"], stamps[0], d_raw)
        so, tb, te = g.decode_scans_dev(d_bag, msg_off, n_points, stamps, lay, 1.0, P["filter_num"], P["blind"], P["voxel_grid_resolution"], d_pts)
        k = g.decode_imu_dev(d_ibag, ioff, d_imus)
        n_msg, n_pk, n_cs = g.imu_split_dev(d_imus, k, te)
        assert n_pk == S and te[0] == te0 and min(n_msg) > 5
        g.first_frame_dev(d_raw, n_raw, te0, 1, d_imus, int(n_msg[0]))
        poses, n_slides = g.run_scans_dev(d_pts, so[1:], tb[1:], 1, n_msg[1:], d_imus + int(n_msg[0]) * IMU_REC, None, d_world)
        # the same run with read-backs
        raw0, pts, recs = np.zeros(n_raw, dtype=synth.POINT_DTYPE), np.zeros(int(so[-1]), dtype=synth.POINT_DTYPE), np.zeros(n_cs, dtype=synth.IMU_DTYPE)
        g.d2h(raw0, d_raw), g.d2h(pts, d_pts), g.d2h(recs, d_imus)
        off = np.r_[0, np.cumsum(n_msg)]
        g_ref.first_frame(raw0, te0, imus=recs[: off[1]])
        w = np.zeros((int(so[-1]), 4), dtype=np.float32)
        g.d2h(w, d_world)
        for s in range(1, S):
            a, b = int(so[s]), int(so[s + 1])
            pr, wr = g_ref.process_scan(pts[a:b], tb[s], imus=recs[off[s]:off[s + 1]], want_world=True)
            _same_pose(poses[s - 1], pr, s)
            assert pr.n_effect > 500, (s, pr.n_effect)
            assert np.array_equal(w[a:b, :3], wr), s
        assert g.get_acc_norm() == g_ref.get_acc_norm()
        _same_handle_state(g, g_ref)
    finally:
        for d in dptrs:
            g.device_free(d)
        _close(g, g_ref)


# ------------------------------------------------------------------ 7. refusals leave the handle untouched
@pytest.mark.gpu
def test_refusals_leave_the_handle_untouched(hip_lib):
    sc = _scene(1)
    scans, tbs, msgs = _config1_run(1)
    short = [s[:400].copy() for s in scans]
    cap = 1 << 15
    g = hip_lib.LegKiloHip(sc.cfg(max_scan_points=cap))
    _start(g, sc, T0 - 0.1)
    g.process_scan(scans[0][:3000], T0 - 0.1)   # a handle in mid-run: counters, times and map have moved
    before = _digest(g)

    def refused(code, names_scan, pts_list, **kw):
        with pytest.raises(hip_lib.LegKiloError, match=rf"error {code}:") as e:
            g.run_scans(pts_list, tbs[: len(pts_list)], **kw)
        if names_scan is not None:
            assert f"scan {names_scan} " in str(e.value), str(e.value)
        assert e.value.n_done == 0
        after = _digest(g)
        assert after[:3] == before[:3], "state or time stamps changed"
        scenes.maps_identical(after[3], before[3])

    bad = [s.copy() for s in short]
    bad[2]["curvature"][200] = bad[2]["curvature"][199] - np.float32(0.002)   # one decreasing curvature in scan 2 of 4
    assert np.all(np.diff(bad[3]["curvature"]) >= 0)
    refused(-1, 2, bad, imus=msgs)
    bad = [s.copy() for s in short]
    bad[2]["curvature"][399] = np.nan
    refused(-1, 2, bad, imus=msgs)
    big = [short[0], np.repeat(scans[1], cap // len(scans[1]) + 1)[: cap + 1], short[2]]   # one point above max_scan_points, still sorted
    assert len(big[1]) == cap + 1
    refused(-3, 1, big)
    refused(-1, 1, [short[0], short[1][:0], short[2]])   # an empty scan
    # n_scans == 0, msg_kind == 3, msg_kind == 1 without n_msg: through the device-pointer entry
    d = g.device_malloc(short[0].nbytes)
    try:
        g.h2d(d, short[0])
        for so, kind, what in ((np.zeros(1, dtype=np.uint64), 0, "n_scans"), (np.array([0, 400], dtype=np.uint64), 3, "msg_kind"),
                               (np.array([0, 400], dtype=np.uint64), 1, "n_msg")):
            with pytest.raises(hip_lib.LegKiloError, match=r"error -1:") as e:
                g.run_scans_dev(d, so, tbs[: len(so) - 1], kind, None, 0)
            assert what in str(e.value), str(e.value)
            after = _digest(g)
            assert after[:3] == before[:3]
            scenes.maps_identical(after[3], before[3])
    finally:
        g.device_free(d)
    # the handle goes on as if nothing had been asked of it
    g_ref = hip_lib.LegKiloHip(sc.cfg(max_scan_points=cap))
    _start(g_ref, sc, T0 - 0.1)
    g_ref.process_scan(scans[0][:3000], T0 - 0.1)
    g.run_scans(short, tbs, imus=msgs)
    _loop(g_ref, short, tbs, 1, msgs)
    _same_handle_state(g, g_ref)
    _close(g, g_ref)


# ------------------------------------------------------------------ 8. CPU
def test_run_options_matches_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "legkilo_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", '
                   'sizeof(lk_run_options), offsetof(lk_run_options, sliding_thresh), offsetof(lk_run_options, half_map_size), '
                   'offsetof(lk_run_options, pad_));return 0;}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    o = abi.lk_run_options
    assert got == [C.sizeof(o), o.sliding_thresh.offset, o.half_map_size.offset, o.pad_.offset] == [16, 0, 8, 12]


def test_live_run_example_and_host_mirror_compile(tmp_path):
    """leg-kilo_amd/host/example_live_run.cc (message bytes -> front ends -> first frame -> KiloPath::runScans -> TUM lines) compiles and
    links against the C-ABI; the symbol it needs is exported and bound."""
    from legkilo_amd import binding

    binding.build()
    assert "lk_run_scans_dev" in binding.EXPORTS and hasattr(C.CDLL(binding.LIB_PATH), "lk_run_scans_dev")
    assert hasattr(binding.LegKiloHip, "run_scans") and hasattr(binding.LegKiloHip, "run_scans_dev")
    src = os.path.join(ROOT, "leg-kilo_amd", "host", "example_live_run.cc")
    exe = str(tmp_path / "lk_live_run_example")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "leg-kilo_amd", "host"),
                        src, "-o", exe, "-L", os.path.join(ROOT, "leg-kilo_amd"), "-llegkilo_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "leg-kilo_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
