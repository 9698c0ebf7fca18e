"""The leg kinematics front end: serialized unitree_legged_msgs/HighState -> lk_kin_imu on the device (lk_decode_highstate(_dev)), the kin branch
of syncPackage (lk_kin_split_dev) and the replay of the records where they lie (lk_batch_replay_scans_kin_dev), against the numpy restatement
in tests/kin_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kin_ref
from legkilo_amd import abi, config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12)
CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)   # test_gpu_parity.py's


def _msg(sec=1, nsec=0, acc_z=1.0, gyr_z=0.5, force=(0, 0, 0, 0), q=0.1, dq=0.2):
    """One HighState message with the given fields (Unitree foot order for force), zeros elsewhere."""
    r = np.zeros(1, dtype=kin_ref.HIGHSTATE_DTYPE)
    r["sec"], r["nsec"] = sec, nsec
    r["acc"][0] = [0.1, 0.2, acc_z]
    r["gyr"][0] = [0.3, 0.4, gyr_z]
    r["force"][0] = force
    r["motor"]["q"][0, :12] = q
    r["motor"]["dq"][0, :12] = dq
    return r.view(np.uint8).reshape(1, -1)


def _msgs(rows):
    return np.concatenate([_msg(**r) for r in rows])


# ------------------------------------------------------------------ CPU: the restatement on hand-traced sequences
def test_contact_detector_inverted_thresholds_toggle_inside_the_window():
    """diter.yaml: T_on = 40 < T_off = 60.  A force held in (40, 60) toggles the state on every update; 30 lifts, 70 lands and holds."""
    d = kin_ref.ContactDetector(40, 60)
    assert [d.update(f) for f in (50, 50, 50, 50, 30, 30, 70, 70, 50)] == [False, True, False, True, False, False, True, True, False]


def test_contact_detector_normal_hysteresis():
    """leg_fusion.yaml: T_on = 220 > T_off = 200.  Inside (200, 220) the state holds; it changes only below 200 / above 220."""
    d = kin_ref.ContactDetector(220, 200)
    assert [d.update(f) for f in (210, 210, 199, 210, 220, 221, 210, 200, 199)] == [True, True, False, False, False, True, True, True, False]


def test_redundancy_dropped_message_still_becomes_previous_and_zero_first_message_is_dropped():
    p = dict(config.DITER, redundancy=True)
    fe = kin_ref.Frontend(p)
    rows = [dict(nsec=0, acc_z=0.0, gyr_z=0.0),       # equals the zero-initialised static: dropped
            dict(nsec=1, acc_z=1.0, gyr_z=2.0),       # kept
            dict(nsec=2, acc_z=1.0, gyr_z=2.0),       # same as previous: dropped
            dict(nsec=3, acc_z=1.0, gyr_z=3.0),       # gyr differs: kept
            dict(nsec=4, acc_z=5.0, gyr_z=3.0),       # acc differs: kept
            dict(nsec=5, acc_z=1.0, gyr_z=2.0),       # equals message 1 and 2, but previous is message 4: kept
            dict(nsec=6, acc_z=1.0, gyr_z=2.0)]       # equals message 5: dropped
    out = fe.process(_msgs(rows))
    assert list(np.round((out["time_stamp"] - 1.0) * 1e9).astype(int)) == [1, 3, 4, 5]
    # the previous message is the last one given, dropped or not
    assert fe.last_acc_z == np.float32(1.0) and fe.last_gyr_z == np.float32(2.0)
    assert fe.process(_msgs([dict(nsec=7, acc_z=1.0, gyr_z=2.0)])).size == 0
    # redundancy off: everything kept
    assert kin_ref.Frontend(dict(p, redundancy=False)).process(_msgs(rows)).size == len(rows)


def test_redundancy_signed_zero_matches_and_nan_never_does():
    fe = kin_ref.Frontend(dict(config.DITER, redundancy=True))
    out = fe.process(_msgs([dict(nsec=0, acc_z=-0.0, gyr_z=0.0),          # -0 == +0: equals the zero static -> dropped
                            dict(nsec=1, acc_z=float("nan"), gyr_z=1.0),  # kept
                            dict(nsec=2, acc_z=float("nan"), gyr_z=1.0)]))  # NaN != NaN -> kept
    assert out.size == 2


def test_contacts_advance_only_on_kept_messages():
    p = dict(config.DITER, redundancy=True)
    fe = kin_ref.Frontend(p)
    f = (50, 50, 50, 50)   # inside (40, 60): toggles per kept message
    out = fe.process(_msgs([dict(nsec=0, acc_z=1.0, force=f), dict(nsec=1, acc_z=1.0, force=f), dict(nsec=2, acc_z=2.0, force=f)]))
    assert out.size == 2 and list(out["contact"][:, 0]) == [0, 1]


def test_leg_order_of_forces_and_motors():
    """Project leg j (FR FL RR RL) reads Unitree foot j ^ 1 and motors 3 (j ^ 1) .. + 2."""
    fe = kin_ref.Frontend(dict(config.LEG_FUSION, redundancy=False))
    m = _msg(force=(0, 300, 0, 300))          # Unitree FR and RR stay on the ground
    hs = kin_ref.read_highstate(m)
    hs["motor"]["q"][0, 3:6] = [0.3, 0.9, -1.7]   # Unitree FR = project leg 0
    out = fe.process(hs.view(np.uint8).reshape(1, -1))
    assert list(out["contact"][0]) == [1, 0, 1, 0]
    q = np.full((4, 3), np.float32(0.1), dtype=np.float64)
    q[0] = np.array([0.3, 0.9, -1.7], dtype=np.float32)
    pos, _, _ = synth.foot_pos_vel(q, np.full((4, 3), np.float32(0.2), dtype=np.float64), config.LEG_FUSION)
    assert np.array_equal(out["foot_pos"][0], pos)


def test_backwards_stamp_is_refused_and_state_kept():
    fe = kin_ref.Frontend(dict(config.DITER, redundancy=False))
    fe.process(_msgs([dict(nsec=5, force=(0, 0, 0, 0))]))
    before = fe.state()
    with pytest.raises(kin_ref.BackwardsStamp):
        fe.process(_msgs([dict(nsec=6, force=(99, 99, 99, 99)), dict(nsec=4)]))
    after = fe.state()
    assert all(np.array_equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("stamps, ends, want", [
    # a front message exactly at e is not taken by that scan (it took nothing before it) but by the next with a larger end
    ([1.0, 2.0, 3.0], [1.0, 2.5], ([0, 2], 2, 2)),
    # two messages at e: the scan takes the run below e and ONE at e; the other goes to the next scan
    ([0.5, 1.0, 1.0, 1.5], [1.0, 1.6], ([2, 0], 1, 2)),   # second scan: newest stamp 1.5 < 1.6 -> not packaged
    ([0.5, 1.0, 1.0, 1.5, 2.0], [1.0, 1.6], ([2, 2], 2, 4)),
    # equal consecutive scan ends: the second takes nothing
    ([0.5, 0.7, 1.0, 1.2], [1.0, 1.0, 1.1], ([3, 0, 0], 3, 3)),
    # ... and at the newest stamp the cache is empty after the first: not packaged
    ([0.5, 1.0], [1.0, 1.0], ([2, 0], 1, 2)),
    # a last scan beyond the newest stamp is not packaged
    ([0.1, 0.2, 0.3], [0.15, 0.25, 0.35], ([1, 1, 0], 2, 2)),
    # nothing before the first end: packaged with no messages
    ([2.0, 3.0], [1.0, 2.5], ([0, 1], 2, 1)),
])
def test_sync_package_edges(stamps, ends, want):
    n_msg, npk, ncs = kin_ref.sync_package(np.array(stamps), np.array(ends))
    n_msg2, npk2, ncs2 = kin_ref.split_cursor(np.array(stamps), np.array(ends))
    assert (list(n_msg), npk, ncs) == (want[0], want[1], want[2])
    assert (list(n_msg2), npk2, ncs2) == (want[0], want[1], want[2])


def test_split_cursor_equals_the_walk_on_random_streams():
    rng = np.random.default_rng(77)
    for _ in range(300):
        t = np.sort(rng.integers(0, 12, rng.integers(0, 14))).astype(np.float64)
        e = np.sort(rng.integers(0, 14, rng.integers(1, 8))).astype(np.float64)
        a, b = kin_ref.sync_package(t, e), kin_ref.split_cursor(t, e)
        assert (list(a[0]), a[1], a[2]) == (list(b[0]), b[1], b[2]), (t, e)


def test_highstate_stream_reads_back_the_generator_values():
    tr = synth.Trajectory()
    msgs, tru = synth.highstate_stream(tr, 3.0, 3.5, config.DITER, hold=10, seed=11)
    assert msgs.shape == (250, abi.LK_HIGHSTATE_BYTES)
    hs = kin_ref.read_highstate(msgs)
    for k in ("sec", "nsec", "acc", "gyr", "force"):
        assert np.array_equal(hs[k], tru[k]), k
    assert np.array_equal(hs["motor"]["q"], tru["q"]) and np.array_equal(hs["motor"]["dq"], tru["dq"])
    # the IMU is held for `hold` messages; the forces dwell inside the window and cross both thresholds
    assert np.array_equal(tru["acc"][0:10], np.repeat(tru["acc"][0:1], 10, 0)) and not np.array_equal(tru["acc"][9], tru["acc"][10])
    f = tru["force"].astype(int)
    assert ((f > 40) & (f < 60)).sum() > 20 and (f < 40).any() and (f > 60).any()
    # bytes the decoder does not read are random (no test passes on zeros)
    assert (msgs[:, 100:110] != 0).mean() > 0.9


def test_new_struct_sizes_match_a_c_compiler(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "legkilo_hip.h"\nint main(void){printf("%zu %zu %zu %zu %d\\n", sizeof(lk_kin_config), '
                   'sizeof(lk_kin_frontend_state), offsetof(lk_kin_config, redundancy), offsetof(lk_kin_frontend_state, last_stamp), '
                   'LK_HIGHSTATE_BYTES);return 0;}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.lk_kin_config), C.sizeof(abi.lk_kin_frontend_state), abi.lk_kin_config.redundancy.offset,
                   abi.lk_kin_frontend_state.last_stamp.offset, abi.LK_HIGHSTATE_BYTES]


def test_kinematics_host_mirror_compiles(tmp_path):
    from legkilo_amd import binding

    binding.build()
    src = os.path.join(ROOT, "leg-kilo_amd", "host", "example_kinematics.cc")
    exe = str(tmp_path / "lk_kin_example")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "leg-kilo_amd", "host"),
                        src, "-o", exe, "-L", os.path.join(ROOT, "leg-kilo_amd"), "-llegkilo_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "leg-kilo_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ------------------------------------------------------------------ GPU
def _handle(hip_lib, params, n_slots=1):
    return hip_lib.LegKiloHip(config.make_config(params, n_slots=n_slots, **SMALL))


def _stream(params, n=51_200, seed=5):
    return synth.highstate_stream(synth.Trajectory(), 2.0, 2.0 + n / 500.0, params, seed=seed)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["diter", "leg_fusion"])
@pytest.mark.parametrize("redundancy", [True, False])
def test_decode_parity_with_the_restatement(hip_lib, name, redundancy):
    p = dict(config.DITER if name == "diter" else config.LEG_FUSION, redundancy=redundancy)
    msgs = _stream(p)
    assert len(msgs) == 51_200
    ref = kin_ref.Frontend(p).process(msgs)
    g = _handle(hip_lib, p)
    try:
        g.kin_configure(p)
        out = g.decode_highstate(msgs)
    finally:
        g.close()
    assert len(out) == len(ref) and (len(ref) < 6000 if redundancy else len(ref) == len(msgs))
    for k in ("time_stamp", "acc", "gyr", "contact"):
        assert np.array_equal(out[k], ref[k]), k
    c = ref["contact"]
    assert 0 < c.mean() < 1 and (np.diff(c, axis=0) != 0).sum() > 100   # the detectors do switch
    dp = np.abs(out["foot_pos"] - ref["foot_pos"]).max()
    dv = np.abs(out["foot_vel"] - ref["foot_vel"]).max()
    print(f"{name} redundancy={redundancy}: {len(out)} kept, max |foot_pos| diff {dp:.3g} m, max |foot_vel| diff {dv:.3g} m/s")
    assert dp <= 1e-14 and dv <= 1e-12, (dp, dv)


@pytest.mark.gpu
def test_host_equals_device_and_chunks_equal_one_call(hip_lib):
    p = dict(config.DITER, redundancy=True)
    msgs = _stream(p, n=20_000, seed=9)
    n = len(msgs)
    g = _handle(hip_lib, p)
    try:
        g.kin_configure(p)
        host = g.decode_highstate(msgs)
        st_host = g.kin_get_frontend()
        g.kin_configure(p)
        d_in = g.device_malloc(msgs.nbytes)
        d_out = g.device_malloc(n * synth.KIN_DTYPE.itemsize)
        g.h2d(d_in, msgs)
        k = g.decode_highstate_dev(d_in, n, d_out)
        dev = np.zeros(k, dtype=synth.KIN_DTYPE)
        g.d2h(dev, d_out)
        st_dev = g.kin_get_frontend()
        assert dev.tobytes() == host.tobytes()
        # 7 uneven chunks, one of them a single message, the device pointer at odd offsets
        g.kin_configure(p)
        cuts = [0, 1, 2, 997, 4001, 4002, 13_333, n]
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            kk = g.decode_highstate_dev(d_in + a * abi.LK_HIGHSTATE_BYTES, b - a, d_out)
            part = np.zeros(kk, dtype=synth.KIN_DTYPE)
            if kk:
                g.d2h(part, d_out)
            parts.append(part)
        st_chunks = g.kin_get_frontend()
        g.device_free(d_in)
        g.device_free(d_out)
    finally:
        g.close()
    assert np.concatenate(parts).tobytes() == host.tobytes()
    ref = kin_ref.Frontend(p)
    ref.process(msgs)
    for st in (st_dev, st_chunks):
        for key in st_host:
            assert np.array_equal(np.asarray(st[key]), np.asarray(st_host[key])), key
    want = ref.state()
    assert list(st_host["contact"]) == list(want["contact"]) and st_host["last_stamp"] == want["last_stamp"]
    assert st_host["last_acc_z"] == want["last_acc_z"] and st_host["last_gyr_z"] == want["last_gyr_z"]


@pytest.mark.gpu
def test_refusals_leave_the_state_alone(hip_lib):
    p = dict(config.LEG_FUSION, redundancy=False)
    msgs = _stream(p, n=400, seed=13)
    g = _handle(hip_lib, p)
    try:
        rc = g.L.lk_decode_highstate(g.h, msgs.ctypes.data_as(C.c_void_p), C.c_size_t(len(msgs)), None, C.byref(C.c_size_t()))
        assert rc == -1   # null output
        out = np.zeros(len(msgs), dtype=synth.KIN_DTYPE)
        rc = g.L.lk_decode_highstate(g.h, msgs.ctypes.data_as(C.c_void_p), C.c_size_t(len(msgs)), out.ctypes.data_as(C.c_void_p), C.byref(C.c_size_t()))
        assert rc == -5   # LK_ERR_STATE: never configured
        assert g.L.lk_kin_get_frontend(g.h, C.byref(abi.lk_kin_frontend_state())) == -5
        g.kin_configure(p)
        g.decode_highstate(msgs[:100])
        before = g.kin_get_frontend()
        # backwards inside the call
        hs = kin_ref.read_highstate(msgs[100:200])
        hs["sec"][50] -= 1
        bad = hs.view(np.uint8).reshape(100, -1)
        with pytest.raises(Exception, match="-1"):
            g.decode_highstate(bad)
        # backwards across calls
        with pytest.raises(Exception, match="-1"):
            g.decode_highstate(msgs[50:60])
        after = g.kin_get_frontend()
        for key in before:
            assert np.array_equal(np.asarray(before[key]), np.asarray(after[key])), key
        # the stream goes on where it was
        rest = g.decode_highstate(msgs[100:])
        ref = kin_ref.Frontend(p)
        ref.process(msgs[:100])
        want = ref.process(msgs[100:])
        for key in ("time_stamp", "contact", "acc", "gyr"):
            assert np.array_equal(rest[key], want[key]), key
        assert np.abs(rest["foot_pos"] - want["foot_pos"]).max() <= 1e-14 and np.abs(rest["foot_vel"] - want["foot_vel"]).max() <= 1e-12
        # split: decreasing scan ends, null pointers
        d = g.device_malloc(264 * 4)
        with pytest.raises(Exception, match="-1"):
            g.kin_split_dev(d, 4, [2.0, 1.0])
        nm = np.zeros(2, dtype=np.uint32)
        a, b = C.c_size_t(), C.c_size_t()
        ends = np.array([1.0, 2.0])
        assert g.L.lk_kin_split_dev(g.h, None, C.c_size_t(4), ends.ctypes.data_as(C.c_void_p), C.c_size_t(2), nm.ctypes.data_as(C.c_void_p),
                                    C.byref(a), C.byref(b)) == -1
        assert g.L.lk_kin_split_dev(g.h, C.c_void_p(d), C.c_size_t(4), None, C.c_size_t(2), nm.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(b)) == -1
        assert g.L.lk_decode_highstate_dev(g.h, None, C.c_size_t(4), C.c_void_p(d), C.byref(a)) == -1
        assert g.L.lk_kin_configure(g.h, None) == -1
        g.device_free(d)
    finally:
        g.close()


@pytest.mark.gpu
def test_split_parity_with_stamps_on_scan_ends(hip_lib):
    p = dict(config.DITER, redundancy=True)
    msgs = _stream(p, n=20_000, seed=21)
    ref = kin_ref.Frontend(p).process(msgs)
    t = ref["time_stamp"]
    rng = np.random.default_rng(3)
    # scan ends: some exactly on a record's stamp (a lone one, or one of two equal stamps), repeated ends, some between records, the last
    # beyond the newest record
    t = t.copy()
    t[100] = t[99]                   # two records at the same stamp
    t[500] = t[501] = t[499]         # three
    ends = np.sort(np.r_[t[rng.choice(len(t), 300, replace=False)], t[99], t[499], t[499], t[1000], t[1000],
                         rng.uniform(t[0] - 0.01, t[-1], 300), t[-1] + 0.001])
    recs = ref.copy()
    recs["time_stamp"] = t
    g = _handle(hip_lib, p)
    try:
        d = g.device_malloc(recs.nbytes)
        g.h2d(d, recs)
        n_msg, npk, ncs = g.kin_split_dev(d, len(recs), ends)
        g.device_free(d)
    finally:
        g.close()
    want = kin_ref.sync_package(t, ends)
    assert (npk, ncs) == (want[1], want[2]) and npk == len(ends) - 1
    assert np.array_equal(n_msg, want[0])
    assert (n_msg == 0).sum() > 10


@pytest.mark.gpu
def test_scratch_grows_and_stays_right(hip_lib):
    """A short stream, a long one, the short one again on one handle (lk_decode_highstate_dev, then lk_kin_split_dev over what it kept, with few and
    with many scans): records, front-end state and split equal, bit for bit, what the same input gives on a fresh handle."""
    p = dict(config.DITER, redundancy=True)
    short, long_ = _stream(p, n=700, seed=31), _stream(p, n=60_000, seed=32)

    def run(g, msgs, n_scans):
        g.kin_configure(p)   # (resets the carried state: every input starts like a first call)
        d_in, d_out = g.device_malloc(msgs.nbytes), g.device_malloc(len(msgs) * synth.KIN_DTYPE.itemsize)
        try:
            g.h2d(d_in, msgs)
            k = g.decode_highstate_dev(d_in, len(msgs), d_out)
            recs = np.zeros(k, dtype=synth.KIN_DTYPE)
            g.d2h(recs, d_out)
            st = g.kin_get_frontend()
            ends = np.linspace(recs["time_stamp"][0], recs["time_stamp"][-1] + 0.01, n_scans)
            n_msg, npk, ncs = g.kin_split_dev(d_out, k, ends)
        finally:
            g.device_free(d_in)
            g.device_free(d_out)
        assert k > 20 and npk > 0 and ncs > 0
        return recs.tobytes(), {key: np.asarray(v).tobytes() for key, v in st.items()}, n_msg.tobytes(), npk, ncs

    one = _handle(hip_lib, p)
    try:
        for msgs, n_scans in ((short, 3), (long_, 2500), (short, 3)):
            fresh = _handle(hip_lib, p)
            try:
                want = run(fresh, msgs, n_scans)
            finally:
                fresh.close()
            assert run(one, msgs, n_scans) == want
    finally:
        one.close()


@pytest.mark.gpu
def test_leg_fusion_recorded_run_from_highstate_bytes(oracle_lib, hip_lib):
    """HighState bytes -> lk_decode_highstate_dev -> lk_kin_split_dev -> lk_batch_replay_scans_kin_dev, the records never leaving HBM, equals the
    oracle's process_scan fed with the restatement's records (counts exact, x to 1e-8, P to 1e-6), and lk_batch_replay_scans_dev fed with the
    same records from the host, bit for bit."""
    import scenes

    P = dict(config.DITER, voxel_grid_resolution=0.3, redundancy=True)
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
    scans, tbs, ends, xs, Ps, streams = [], [], [], [], [], []
    for s in range(S):
        tb = t0 + 0.5 + 0.13 * s
        scans.append(scenes.vlp_scan_input(sc, tb, 80 + s))
        tbs.append(tb)
        ends.append(tb + float(scans[-1]["curvature"][-1]))
        xs.append(synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5))
        Ps.append(1e-4 * np.eye(30))
        streams.append(synth.highstate_stream(sc.traj, tb, ends[-1], P, hold=2, seed=700 + s)[0])   # the scan's own window
    streams.append(synth.highstate_stream(sc.traj, ends[-1] + 0.004, ends[-1] + 0.02, P, hold=2, seed=799)[0])   # newer than the last end
    msgs = np.concatenate(streams)
    ref = kin_ref.Frontend(P).process(msgs)
    n_ref, npk, ncs = kin_ref.sync_package(ref["time_stamp"], ends)
    assert npk == S and min(n_ref) > 10
    g = hip_lib.LegKiloHip(sc.cfg(n_slots=S))
    try:
        g.map_import(blob)
        g.init_process_cov_q()
        g.set_acc_norm(9.81)
        o.set_acc_norm(9.81)
        g.kin_configure(P)
        d_msgs = g.device_malloc(msgs.nbytes)
        d_kins = g.device_malloc(len(msgs) * synth.KIN_DTYPE.itemsize)
        g.h2d(d_msgs, msgs)
        k = g.decode_highstate_dev(d_msgs, len(msgs), d_kins)
        n_msg, n_pk, n_cs = g.kin_split_dev(d_kins, k, ends)
        assert (k, n_pk, n_cs) == (len(ref), npk, ncs) and np.array_equal(n_msg, n_ref)
        allp = np.ascontiguousarray(np.concatenate(scans))
        so = np.r_[0, np.cumsum([len(x) for x in scans])]
        d_pts = g.device_malloc(allp.nbytes)
        g.h2d(d_pts, allp)
        g.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        ps = g.batch_replay_scans_kin_dev(d_pts, so, tbs, n_msg, d_kins)
        dev_states = [g.get_state(slot=s) for s in range(S)]
        # the same records through the host
        recs = np.zeros(n_cs, dtype=synth.KIN_DTYPE)
        g.d2h(recs, d_kins)
        for key in ("time_stamp", "contact", "acc", "gyr"):
            assert np.array_equal(recs[key], ref[key][:n_cs]), key
        per = np.split(recs, np.cumsum(n_msg)[:-1])
        g.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        ph = g.batch_replay_scans_dev(d_pts, so, tbs, kins=per)
        host_states = [g.get_state(slot=s) for s in range(S)]
        for d in (d_msgs, d_kins, d_pts):
            g.device_free(d)
        off = np.r_[0, np.cumsum(n_ref)]
        for s in range(S):
            assert bytes(ps[s]) == bytes(ph[s]), s
            assert dev_states[s][0].tobytes() == host_states[s][0].tobytes() and dev_states[s][1].tobytes() == host_states[s][1].tobytes(), s
            o.set_state(xs[s], Ps[s])
            o.set_times(tbs[s], tbs[s])
            po, _ = o.process_scan(scans[s], tbs[s], kins=ref[off[s]:off[s + 1]])
            xo, Po = o.get_state()
            xg, Pg = dev_states[s]
            assert (po.n_buckets, po.n_updates, po.n_effect) == (ps[s].n_buckets, ps[s].n_updates, ps[s].n_effect), s
            assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (s, np.abs(xo - xg).max())
            assert np.allclose(Po, Pg, rtol=1e-6, atol=1e-11), (s, np.abs(Po - Pg).max())
    finally:
        g.close()
