"""The lidar front end of a recorded run in one call: a run's PointCloud2 payloads in HBM -> decoded, voxel-grid filtered, time-sorted scans
(lk_decode_scans_dev), against the per-scan chain lk_decode_scan_dev + lk_preprocess_scan_dev on the same bytes (bit for bit), the oracle's
decode + preprocess, and - chained with the leg kinematics front end - the oracle's process_scan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudcases as cc
import preprocess_oracle as po
import scenes
from legkilo_amd import config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12)
CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)   # test_gpu_parity.py's
PT = synth.POINT_DTYPE.itemsize


def _run(scene, n, t0=2.0, seed=0, cut=True):
    """n VLP-16 scans 0.1 s apart as POINT_DTYPE with curvature = time offset; cut=True: each cut to a length of its own."""
    out = []
    for k in range(n):
        pts = synth.vlp16_scan(scene.world, scene.traj, t0 + 0.1 * k, scene.P, seed_noise=3003 + seed + k)
        out.append(pts[: int(len(pts) * (0.35 + 0.65 * ((k * 7) % 10) / 9))] if cut else pts)
    return out


def _messages(scans, lidar_type, t0=2.0, seed=0):
    stamps = t0 + 0.1 * np.arange(len(scans))
    msgs = [synth.cloud_message(sc, lidar_type, float(stamps[k]), seed=seed + k) for k, sc in enumerate(scans)]
    buf, msg_off, n_points = synth.pack_cloud_run(msgs, seed=seed)
    return msgs, buf, msg_off, n_points, stamps


# ------------------------------------------------------------------ CPU
def test_new_symbols_are_exported_and_bound():
    import __graft_entry__ as ge
    from legkilo_amd import binding

    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    for name in ("lk_decode_scans_dev", "lk_decode_scan_dev"):
        assert name in ge.declared_symbols() and name in binding.EXPORTS and hasattr(lib, name), name
    assert hasattr(binding.LegKiloHip, "decode_scans_dev") and hasattr(binding.LegKiloHip, "decode_scan_dev")


def test_lidar_host_mirror_compiles(tmp_path):
    from legkilo_amd import binding

    binding.build()
    src = os.path.join(ROOT, "leg-kilo_amd", "host", "example_lidar_frontend.cc")
    exe = str(tmp_path / "lk_lidar_example")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "leg-kilo_amd", "host"),
                        src, "-o", exe, "-L", os.path.join(ROOT, "leg-kilo_amd"), "-llegkilo_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "leg-kilo_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_packed_run_reads_back_at_the_stated_offsets(lidar_type):
    rng = np.random.default_rng(lidar_type)
    scans = []
    for _ in range(9):
        pts = np.zeros(int(rng.integers(50, 400)), dtype=synth.POINT_DTYPE)
        for f in ("x", "y", "z"):
            pts[f] = rng.normal(0, 10, len(pts))
        pts["curvature"] = np.sort(rng.uniform(0, 0.1, len(pts))).astype(np.float32)
        scans.append(pts)
    msgs, buf, msg_off, n_points, stamps = _messages(scans, lidar_type, t0=5.0, seed=11)
    lay = synth.cloud_layout(lidar_type)
    dt = synth.CLOUD_DTYPES[lidar_type]
    assert dt == {1: po.VELODYNE_DTYPE, 2: po.OUSTER_DTYPE, 3: po.HESAI_DTYPE}[lidar_type] and lay["point_step"] == dt.itemsize
    assert len(set(n_points.tolist())) > 5 and np.all(msg_off % 2 == 1) and np.all(np.diff(stamps) > 0)
    ends = msg_off + n_points.astype(np.uint64) * dt.itemsize
    assert np.all(msg_off[1:] > ends[:-1])   # gaps between the messages
    for k, sc in enumerate(scans):
        b = buf[int(msg_off[k]):int(ends[k])]
        raw = np.frombuffer(b.tobytes(), dtype=dt)
        assert np.array_equal(raw.view(np.uint8), msgs[k].view(np.uint8)) and len(raw) == n_points[k]
        rows = b.reshape(-1, dt.itemsize)
        for f in ("x", "y", "z"):
            o = lay["off_" + f]
            assert np.array_equal(rows[:, o:o + 4].copy().view("<f4")[:, 0], sc[f]), f
        # the field the handler reads, at the layout's offset, gives back the generator's time offsets
        t = rows[:, lay["off_time"]:]
        tt = t[:, :8].copy().view("<f8")[:, 0] if lidar_type == 3 else t[:, :4].copy().view("<u4" if lidar_type == 2 else "<f4")[:, 0]
        got = tt.astype(np.float64) * synth.CLOUD_TIME_SCALE[lidar_type] - (stamps[k] if lidar_type == 3 else 0.0)
        assert np.allclose(got, sc["curvature"], atol=1e-6), k


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def scene():
    return scenes.Scene(**SMALL)


@pytest.fixture(scope="module")
def run9(scene):
    return _run(scene, 9)


class _Dev:
    """A handle with room for a packed run in HBM, output room for the batch entry and scratch for the per-scan chain."""

    def __init__(self, hip_lib, scene, buf_bytes, n_max, total):
        self.g = hip_lib.LegKiloHip(scene.cfg())
        self.d_msgs = self.g.device_malloc(buf_bytes)
        self.d_out = self.g.device_malloc(total * PT)
        self.d_dec = self.g.device_malloc(n_max * PT)
        self.d_ds = self.g.device_malloc(n_max * PT)

    def batch(self, msg_off, n_points, stamps, layout, scale, fn, blind, leaf):
        so, tb, te = self.g.decode_scans_dev(self.d_msgs, msg_off, n_points, stamps, layout, scale, fn, blind, leaf, self.d_out)
        out = np.zeros(int(so[-1]), dtype=synth.POINT_DTYPE)
        self.g.d2h(out, self.d_out)
        return [out[so[s]:so[s + 1]] for s in range(len(so) - 1)], tb, te, so

    def per_scan(self, msg_off, n_points, stamps, layout, scale, fn, blind, leaf):
        outs, tbs, tes = [], [], []
        for s in range(len(msg_off)):
            n, tb, te = self.g.decode_scan_dev(self.d_msgs + int(msg_off[s]), int(n_points[s]), layout, scale, fn, blind, float(stamps[s]), self.d_dec)
            nd = self.g.preprocess_scan_dev(self.d_dec, n, leaf, self.d_ds)
            o = np.zeros(nd, dtype=synth.POINT_DTYPE)
            self.g.d2h(o, self.d_ds)
            outs.append(o), tbs.append(tb), tes.append(te)
        return outs, np.array(tbs), np.array(tes)

    def close(self):
        for d in (self.d_msgs, self.d_out, self.d_dec, self.d_ds):
            self.g.device_free(d)
        self.g.close()


def _dev_for(hip_lib, scene, buf, n_points):
    dev = _Dev(hip_lib, scene, buf.nbytes, int(n_points.max()), int(n_points.sum()))
    dev.g.h2d(dev.d_msgs, buf)
    return dev


def _assert_equal_chain(dev, tables, layout, scale, fn, blind, leaf):
    msg_off, n_points, stamps = tables
    got, tb, te, so = dev.batch(msg_off, n_points, stamps, layout, scale, fn, blind, leaf)
    want, wb, we = dev.per_scan(msg_off, n_points, stamps, layout, scale, fn, blind, leaf)
    assert so[0] == 0 and len(got) == len(want) == len(msg_off)
    for s in range(len(want)):
        assert len(got[s]) == len(want[s]) > 0, (s, len(got[s]), len(want[s]))
        assert got[s].tobytes() == want[s].tobytes(), (s, int((got[s] != want[s]).sum()))
    assert np.array_equal(tb, wb) and np.array_equal(te, we), (tb - wb, te - we)
    return got, tb, te, so


@pytest.mark.gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
@pytest.mark.parametrize("filter_num", [1, 3])
@pytest.mark.parametrize("leaf", [0.3, 0.5])
def test_batch_equals_the_per_scan_chain(hip_lib, scene, run9, lidar_type, filter_num, leaf):
    _, buf, msg_off, n_points, stamps = _messages(run9, lidar_type, seed=lidar_type)
    layout, scale = synth.cloud_layout(lidar_type), synth.CLOUD_TIME_SCALE[lidar_type]
    dev = _dev_for(hip_lib, scene, buf, n_points)
    try:
        got, tb, te, so = _assert_equal_chain(dev, (msg_off, n_points, stamps), layout, scale, filter_num, 1.5, leaf)
    finally:
        dev.close()
    assert len(set(n_points.tolist())) == len(run9)
    for s in range(len(got)):
        assert np.all(np.diff(got[s]["curvature"]) >= 0)
    assert np.all(tb >= stamps) and np.all(tb < stamps + 0.1) and np.all(te > tb)   # Hesai: absolute stamps, the others header + offset


@pytest.mark.gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_batch_equals_the_oracle(hip_lib, scene, run9, lidar_type):
    scans = [sc[:n] for sc, n in zip(run9[:3], (1800, 2500, 2100))]
    msgs, buf, msg_off, n_points, stamps = _messages(scans, lidar_type, seed=30 + lidar_type)
    layout, scale = synth.cloud_layout(lidar_type), synth.CLOUD_TIME_SCALE[lidar_type]
    dev = _dev_for(hip_lib, scene, buf, n_points)
    try:
        got, tb, te, _ = dev.batch(msg_off, n_points, stamps, layout, scale, 3, 1.5, 0.3)
    finally:
        dev.close()
    for s, raw in enumerate(msgs):
        dec, b, e = po.decode(raw, lidar_type, scale, 3, 1.5, header_stamp=float(stamps[s]))
        want = po.preprocess(dec, 0.3)
        assert len(got[s]) == len(want) > 100 and got[s].tobytes() == want.tobytes(), s
        assert (tb[s], te[s]) == (b, e), s


@pytest.mark.gpu
def test_refusals_name_the_message_and_leave_the_handle_usable(hip_lib, scene, run9):
    scans = [sc[:3000] for sc in run9[:5]]
    layout, scale = synth.cloud_layout(1), 1.0

    def tables(mutate=None):
        sc = [s.copy() for s in scans]
        if mutate:
            mutate(sc)
        return _messages(sc, 1, seed=7)[1:]

    def blind_all(sc):   # every point of message 2 inside the blind radius
        sc[2]["x"], sc[2]["y"], sc[2]["z"] = 0.1, 0.2, 0.3

    def far(sc):          # one point of message 1 at 1e5 m in x and y: its voxel index overflows at leaf 0.3, the others' does not
        sc[1]["x"][0], sc[1]["y"][0] = 1.0e5, -1.0e5

    buf0, off0, np0, st0 = tables()
    st_back = st0.copy()
    st_back[4] = st0[3] - 0.05
    cases = [(buf0, off0, np.where(np.arange(5) == 3, 0, np0).astype(np.uint32), st0, layout, r"message 3 has no points"),
             tables(blind_all) + (layout, r"message 2 decodes to no points"),
             (buf0, off0, np0, st_back, layout, r"message 4: header stamp older than message 3"),
             tables(far) + (layout, r"message 1: voxel grid leaf too small"),
             (buf0, off0, np0, st0, dict(layout, lidar_type=4), r"lidar_type must be 1, 2 or 3"),
             (buf0, off0, np0, st0, dict(layout, off_time=20), r"field offsets exceed point_step")]
    dev = _Dev(hip_lib, scene, max(c[0].nbytes for c in cases), int(np0.max()), int(np0.sum()))
    try:
        for b, o, n, s, lay, msg in cases:
            dev.g.h2d(dev.d_msgs, b)
            with pytest.raises(hip_lib.LegKiloError, match=r"error -1: .*" + msg):
                dev.g.decode_scans_dev(dev.d_msgs, o, n, s, lay, scale, 1, 1.5, 0.3, dev.d_out)
            # the same handle, a valid run: equals the per-scan chain
            dev.g.h2d(dev.d_msgs, buf0)
            _assert_equal_chain(dev, (off0, np0, st0), layout, scale, 1, 1.5, 0.3)
        for fn, leaf in ((0, 0.3), (1, 0.0), (1, float("nan"))):
            with pytest.raises(hip_lib.LegKiloError, match="error -1: .*bad argument"):
                dev.g.decode_scans_dev(dev.d_msgs, off0, np0, st0, layout, scale, fn, 1.5, leaf, dev.d_out)
        _assert_equal_chain(dev, (off0, np0, st0), layout, scale, 3, 1.5, 0.5)
    finally:
        dev.close()


@pytest.mark.gpu
def test_pools_grow_and_stay_right(hip_lib, scene, run9):
    """A small batch, a large batch, the small batch again on one handle: each equals the per-scan chain."""
    small = _messages(run9[:2], 2, seed=3)[1:]
    large = _messages(run9 + _run(scene, 4, t0=3.0, seed=50, cut=False), 2, seed=4)[1:]
    layout, scale = synth.cloud_layout(2), synth.CLOUD_TIME_SCALE[2]
    dev = _Dev(hip_lib, scene, large[0].nbytes, int(large[2].max()), int(large[2].sum()))
    try:
        for buf, msg_off, n_points, stamps in (small, large, small):
            dev.g.h2d(dev.d_msgs, buf)
            _assert_equal_chain(dev, (msg_off, n_points, stamps), layout, scale, 3, 1.5, 0.3)
    finally:
        dev.close()


@pytest.mark.gpu
def test_bag_bytes_to_poses_leg_fusion_and_imu(oracle_lib, hip_lib):
    """PointCloud2 bytes -> lk_decode_scans_dev; HighState bytes -> lk_decode_highstate_dev; lk_kin_split_dev on the new end times;
    lk_batch_replay_scans_kin_dev - only tables leave HBM.  Counts equal the oracle's process_scan fed with oracle-decoded scans (x to 1e-8),
    poses and states equal the same replay on the per-scan GPU chain's scans bit for bit; then the same scans in IMU mode
    (lk_batch_replay_scans_dev with host IMU records) against the oracle in only_imu_use mode."""
    import kin_ref

    P = dict(config.DITER, lidar_type=1, time_scale=1.0, filter_num=3, blind=1.5, voxel_grid_resolution=0.3, redundancy=True)
    sc = scenes.Scene(params=P, **CAPS)
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=False)
    t0 = 2.0
    x0 = scenes.init_filter(o, sc, t0)
    scenes.first_frame(o, sc, t0, x0)
    scenes.replay_vlp(o, sc, t0, 4, use_kin=True)
    blob = o.map_export()
    o.set_map_insert(False)
    rng = np.random.default_rng(4343)
    S = 6
    stamps = [t0 + 0.5 + 0.13 * s for s in range(S)]
    msgs = [synth.cloud_message(synth.vlp16_scan(sc.world, sc.traj, tb, P, seed_noise=3083 + s), 1, tb, seed=s) for s, tb in enumerate(stamps)]
    buf, msg_off, n_points = synth.pack_cloud_run(msgs, seed=5)
    ref_scans, ref_tb, ref_te = [], [], []
    for s, m in enumerate(msgs):
        dec, b, e = po.decode_vec(m, 1, 1.0, P["filter_num"], P["blind"], header_stamp=stamps[s])
        ref_scans.append(po.preprocess(dec, P["voxel_grid_resolution"]))
        ref_tb.append(b), ref_te.append(e)
    xs = [synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5) for tb in ref_tb]
    Ps = [1e-4 * np.eye(30)] * S
    streams = [synth.highstate_stream(sc.traj, ref_tb[s], ref_te[s], P, hold=2, seed=700 + s)[0] for s in range(S)]
    streams.append(synth.highstate_stream(sc.traj, ref_te[-1] + 0.004, ref_te[-1] + 0.02, P, hold=2, seed=799)[0])   # newer than the last end
    hs = np.concatenate(streams)
    kref = kin_ref.Frontend(P).process(hs)
    n_ref, npk, ncs = kin_ref.sync_package(kref["time_stamp"], ref_te)
    assert npk == S and min(n_ref) > 10
    g = hip_lib.LegKiloHip(sc.cfg(n_slots=S))
    dptrs = []
    try:
        g.map_import(blob)
        g.init_process_cov_q()
        g.set_acc_norm(9.81)
        o.set_acc_norm(9.81)
        g.kin_configure(P)
        total, n_max = int(n_points.sum()), int(n_points.max())
        dptrs = [g.device_malloc(nb) for nb in (buf.nbytes, total * PT, hs.nbytes, len(hs) * synth.KIN_DTYPE.itemsize, n_max * PT, n_max * PT, total * PT)]
        d_bag, d_pts, d_hs, d_kins, d_dec, d_ds, d_pts2 = dptrs
        g.h2d(d_bag, buf)
        g.h2d(d_hs, hs)
        # bag bytes -> poses in four calls
        so, tb, te = g.decode_scans_dev(d_bag, msg_off, n_points, stamps, synth.cloud_layout(1), 1.0, P["filter_num"], P["blind"],
                                        P["voxel_grid_resolution"], d_pts)
        k = g.decode_highstate_dev(d_hs, len(hs), d_kins)
        n_msg, n_pk, n_cs = g.kin_split_dev(d_kins, k, te)
        g.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        ps = g.batch_replay_scans_kin_dev(d_pts, so, tb, n_msg, d_kins)
        dev_states = [g.get_state(slot=s) for s in range(S)]
        assert list(tb) == ref_tb and list(te) == ref_te
        assert (k, n_pk, n_cs) == (len(kref), npk, ncs) and np.array_equal(n_msg, n_ref)
        got = np.zeros(int(so[-1]), dtype=synth.POINT_DTYPE)
        g.d2h(got, d_pts)
        for s in range(S):
            assert got[so[s]:so[s + 1]].tobytes() == ref_scans[s].tobytes(), s
        # the same replay on the scans of the per-scan GPU chain
        chain, tb2 = [], []
        for s in range(S):
            n, b, _ = g.decode_scan_dev(d_bag + int(msg_off[s]), int(n_points[s]), synth.cloud_layout(1), 1.0, P["filter_num"], P["blind"], stamps[s], d_dec)
            nd = g.preprocess_scan_dev(d_dec, n, P["voxel_grid_resolution"], d_ds)
            part = np.zeros(nd, dtype=synth.POINT_DTYPE)
            g.d2h(part, d_ds)
            chain.append(part), tb2.append(b)
        g.h2d(d_pts2, np.concatenate(chain))
        g.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        ph = g.batch_replay_scans_kin_dev(d_pts2, np.r_[0, np.cumsum([len(c) for c in chain])], tb2, n_msg, d_kins)
        chain_states = [g.get_state(slot=s) for s in range(S)]
        recs = np.zeros(n_cs, dtype=synth.KIN_DTYPE)
        g.d2h(recs, d_kins)
        per = np.split(recs, np.cumsum(n_msg)[:-1])
        for s in range(S):
            assert bytes(ps[s]) == bytes(ph[s]), s
            assert dev_states[s][0].tobytes() == chain_states[s][0].tobytes() and dev_states[s][1].tobytes() == chain_states[s][1].tobytes(), s
            o.set_state(xs[s], Ps[s])
            o.set_times(ref_tb[s], ref_tb[s])
            po_, _ = o.process_scan(ref_scans[s], ref_tb[s], kins=per[s])
            xo, Po = o.get_state()
            xg, Pg = dev_states[s]
            assert (po_.n_buckets, po_.n_updates, po_.n_effect) == (ps[s].n_buckets, ps[s].n_updates, ps[s].n_effect), s
            assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (s, np.abs(xo - xg).max())
            assert np.allclose(Po, Pg, rtol=1e-6, atol=1e-11), (s, np.abs(Po - Pg).max())
        # IMU mode (only_imu_use, KILO.cc:379-383): the same device scans, host IMU records
        oi = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
        oi.map_import(blob)
        oi.set_map_insert(False)
        oi.init_process_cov_q()
        oi.set_acc_norm(9.81)
        imus = [synth.imu_stream(sc.traj, ref_tb[s], ref_te[s], seed=8600 + s) for s in range(S)]
        g.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        pi = g.batch_replay_scans_dev(d_pts, so, tb, imus=imus)
        for s in range(S):
            oi.set_state(xs[s], Ps[s])
            oi.set_times(ref_tb[s], ref_tb[s])
            po_, _ = oi.process_scan(ref_scans[s], ref_tb[s], imus=imus[s])
            xo, Po = oi.get_state()
            xg, Pg = g.get_state(slot=s)
            assert (po_.n_buckets, po_.n_updates, po_.n_effect) == (pi[s].n_buckets, pi[s].n_updates, pi[s].n_effect), s
            assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (s, np.abs(xo - xg).max())
            assert np.allclose(Po, Pg, rtol=1e-6, atol=1e-11), (s, np.abs(Po - Pg).max())
        oi.close()
    finally:
        for d in dptrs:
            g.device_free(d)
        g.close()


# ------------------------------------------------------------------ one body for a scan and a run
def _oracle(raw, lidar_type, fn, blind, leaf, stamp):
    dec, b, e = po.decode(raw, lidar_type, cc.SCALE[lidar_type], fn, blind, header_stamp=float(stamp))
    return dec, po.preprocess(dec, leaf), b, e


def _assert_run_equals_oracle_and_chain(dev, msgs, lidar_type, fn, blind, leaf, seed=0, chain=True):
    """lk_decode_scans_dev on msgs == po.decode + po.preprocess per message (bits) == the per-scan entries on the same device bytes."""
    buf, msg_off, n_points = synth.pack_cloud_run(msgs, seed=seed)
    stamps = cc.run_stamps(len(msgs))
    layout, scale = synth.cloud_layout(lidar_type), cc.SCALE[lidar_type]
    dev.g.h2d(dev.d_msgs, buf)
    got, tb, te, so = dev.batch(msg_off, n_points, stamps, layout, scale, fn, blind, leaf)
    want = [_oracle(m, lidar_type, fn, blind, leaf, stamps[s]) for s, m in enumerate(msgs)]
    assert [int(v) for v in so] == [0] + [int(v) for v in np.cumsum([len(w[1]) for w in want])]
    for s, (_, w, b, e) in enumerate(want):
        assert got[s].tobytes() == w.tobytes(), (s, len(got[s]), len(w))
        assert (tb[s], te[s]) == (b, e), s
    if chain:
        outs, cb, ce = dev.per_scan(msg_off, n_points, stamps, layout, scale, fn, blind, leaf)
        for s in range(len(msgs)):
            assert outs[s].tobytes() == got[s].tobytes(), s
        assert np.array_equal(cb, tb) and np.array_equal(ce, te)
    return want


@pytest.fixture(scope="module")
def tied_cloud():
    """20 610 points at leaf 0.5: ten copies, 16 m apart in x, of cloudcases' order_visible (cells of 3 .. 300 points whose float32 sums depend on
    the order) and stamps (one cell per lattice site) clouds.  Sent with cc.as_message its stamps are the 50 bins of 2 ms: the time sort meets
    runs of equal keys, and the single-block radix sort (up to 1 024 pairs) holds neither the points nor the cells."""
    leaf = 0.5
    base = np.concatenate([cc.grid_case(f"order_visible[{leaf}]").pts, cc.grid_case(f"stamps[{leaf}]").pts])
    copies = []
    for k in range(10):
        c = base.copy()
        c["x"] = (c["x"].astype(np.float64) + 32 * leaf * k).astype(np.float32)
        copies.append(c)
    return np.concatenate(copies), leaf


@pytest.mark.gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_one_message_runs_take_the_other_sort(hip_lib, scene, run9, tied_cloud, lidar_type):
    """A run of ONE message goes through the device-wide sort, not the segmented one: 1, 255, 256, 257 and 1 025 points (every point kept, so
    the sorts see these sizes: either side of a block and of the single-block sort's 1 024), and one message of 20 610 points with full cells and
    tied stamps.  Each equals the oracle and the per-scan entries bit for bit."""
    big, big_leaf = tied_cloud
    assert len(big) > 20000
    dev = _Dev(hip_lib, scene, len(big) * 64, len(big), len(big))
    try:
        for n in (1, 255, 256, 257, 1025):
            raw = synth.cloud_message(run9[1][:n], lidar_type, 100.0, seed=n)
            want = _assert_run_equals_oracle_and_chain(dev, [raw], lidar_type, 1, 0.0, 0.3, seed=n)
            assert len(want[0][0]) == n
        want = _assert_run_equals_oracle_and_chain(dev, [cc.as_message(big, lidar_type, seed=5)], lidar_type, 1, 0.0, big_leaf, seed=6)
        dec, out = want[0][0], want[0][1]
        assert len(dec) == len(big) and 1024 < len(out) < len(dec) // 4                  # several points per cell
        assert len(np.unique(out["curvature"])) < len(out) // 4                          # stamps tie in groups
    finally:
        dev.close()


def _in_cell(n, cell, seed, leaf=0.5):
    rng = np.random.default_rng(seed)
    pts = np.zeros(n, dtype=synth.POINT_DTYPE)
    xyz = (np.array(cell) + rng.uniform(0.1, 0.9, size=(n, 3))) * leaf
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return pts


@pytest.mark.gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_two_message_boundary(hip_lib, scene, lidar_type):
    """Runs of (1, 257) and (257, 1) points whose cell keys are equal on both sides of the scan boundary (keys count from each scan's own
    minimum): two scans, so the message ids must decide - taken for one scan, the boundary cells would merge and share one set of bounds."""
    one = _in_cell(1, (4, 2, 1), 1)
    two_cells = np.concatenate([_in_cell(128, (0, 0, 0), 2), _in_cell(129, (1, 0, 0), 3)])[::-1].copy()
    one_cell = _in_cell(257, (1, 1, 0), 4)
    runs = ([one, two_cells], [one_cell, one])
    for a, b in runs:
        assert cc.sorted_keys(a, 0.5)[-1] == cc.sorted_keys(b, 0.5)[0] == 0
    dev = _Dev(hip_lib, scene, 258 * 64, 257, 258)
    try:
        for k, clouds in enumerate(runs):
            want = _assert_run_equals_oracle_and_chain(dev, [cc.as_message(c, lidar_type, seed=s) for s, c in enumerate(clouds)], lidar_type, 1, 0.0, 0.5,
                                                       seed=k)
            assert [len(w[1]) for w in want] == ([1, 2], [1, 1])[k]
    finally:
        dev.close()


def _small_first_frame(g, scene, t0=2.0):
    """The filter at the scene's state at t0 and a small map under it (2 500 points of a static scan): what lk_process_raw_scan needs."""
    x0 = scenes.init_filter(g, scene, t0)
    raw = synth.vlp16_scan(scene.world, scenes.Frozen(scene.traj, t0), t0, scene.P)[::11][:2500]
    xb = scenes.xyz_of(raw)
    g.map_build(scenes.world_of(x0, xb, scene.P), xb)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [False, True])
def test_the_shared_pool_keeps_its_promises(hip_lib, scene, run9, monkeypatch, poison):
    """One handle, one scratch pool for every front-end entry: a 7-message run, lk_preprocess_scan_dev on 300 points, the run again, the host
    wrappers on a message larger than anything seen (the pool regrows, the staging arrays move), lk_process_raw_scan.  Every output equals the
    oracle's bit for bit, the pose a fresh handle's.  Once more with fresh pools full of 0x5a bytes."""
    if poison:
        monkeypatch.setenv("LEGKILO_POISON_POOLS", "1")
    else:
        monkeypatch.delenv("LEGKILO_POISON_POOLS", raising=False)
    lt, fn, blind, leaf = 1, 3, 0.0, 0.3
    sizes = [1, 257, 2, 256, 255, 1025, 64]
    msgs = [synth.cloud_message(run9[k][100 * k:100 * k + n], lt, 100.0 + 0.1 * k, seed=40 + k) for k, n in enumerate(sizes)]
    big = synth.cloud_message(run9[8], lt, 101.0, seed=48)
    assert len(big) > 4 * sum(sizes)
    big_dec, big_out, big_b, big_e = _oracle(big, lt, fn, 1.5, leaf, 101.0)
    pre = synth.preprocess_velodyne(synth.vlp16_scan(scene.world, scene.traj, 2.1, scene.P, seed_noise=3004), 3, 1.5)[:3000]
    imus = synth.imu_stream(scene.traj, 2.1, 2.2, seed=3004)
    fresh = hip_lib.LegKiloHip(scene.cfg())
    try:
        _small_first_frame(fresh, scene)
        want_pose, want_nd = fresh.process_raw_scan(pre, leaf, 2.1, imus=imus)
        want_x = fresh.get_state()[0]
    finally:
        fresh.close()
    dev = _Dev(hip_lib, scene, sum(sizes) * 64, max(sizes), sum(sizes))
    try:
        g = dev.g
        _small_first_frame(g, scene)
        _assert_run_equals_oracle_and_chain(dev, msgs, lt, fn, blind, leaf, seed=9, chain=False)
        pts300 = run9[7][:300]
        g.h2d(dev.d_dec, pts300)
        n300 = g.preprocess_scan_dev(dev.d_dec, 300, leaf, dev.d_ds)
        got300 = np.zeros(n300, dtype=synth.POINT_DTYPE)
        g.d2h(got300, dev.d_ds)
        assert got300.tobytes() == po.preprocess(pts300, leaf).tobytes()
        _assert_run_equals_oracle_and_chain(dev, msgs, lt, fn, blind, leaf, seed=9, chain=False)
        dec, b, e = g.decode_scan(big.tobytes(), len(big), synth.cloud_layout(lt), cc.SCALE[lt], fn, 1.5, header_stamp=101.0)
        assert dec.tobytes() == big_dec.tobytes() and (b, e) == (big_b, big_e)
        assert g.preprocess_scan(dec, leaf).tobytes() == big_out.tobytes() and len(big_out) > sum(sizes)
        pose, nd = g.process_raw_scan(pre, leaf, 2.1, imus=imus)
        assert nd == want_nd == len(po.preprocess(pre, leaf)) and bytes(pose) == bytes(want_pose)
        assert g.get_state()[0].tobytes() == want_x.tobytes()
    finally:
        dev.close()
