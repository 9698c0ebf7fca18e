"""The IMU front end: serialized sensor_msgs/Imu -> lk_imu on the device (lk_decode_imu(_dev)), the IMU branch of syncPackage
(lk_imu_split_dev) and an IMU-only recorded run from message bytes (lk_first_frame_dev + lk_batch_replay_scans_imu_dev), against the numpy
restatement in tests/imu_ref.py and the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import imu_ref
import kin_ref
from legkilo_amd import abi, config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12)
CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)   # test_kin_frontend.py's
REC = synth.IMU_DTYPE.itemsize


def _params(redundancy):
    return dict(config.LEG_FUSION, only_imu_use=True, redundancy=redundancy)


def _imus(rows, t0=7.0):
    """IMU_DTYPE records from (acc_z, gyr_z) pairs, 5 ms apart."""
    r = np.zeros(len(rows), dtype=synth.IMU_DTYPE)
    r["stamp"] = t0 + 0.005 * np.arange(len(rows))
    r["acc"][:, :2], r["gyr"][:, :2] = [0.1, 0.2], [0.3, 0.4]
    r["acc"][:, 2], r["gyr"][:, 2] = [a for a, _ in rows], [g for _, g in rows]
    return r


def _stream(n, seed, t0=100.0):
    """n records at 200 Hz whose z values are held over runs of 1 .. 4 messages (one run covers messages 250 .. 260: a 256-message block
    edge), serialized with frame_id lengths 0 .. 40 mixed per message.  -> (records, buf, msg_off)"""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=synth.IMU_DTYPE)
    r["stamp"] = t0 + 0.005 * np.arange(n) + rng.uniform(0, 0.001, n)
    r["acc"], r["gyr"] = rng.normal(0, 3, (n, 3)) + [0, 0, 9.8], rng.normal(0, 0.2, (n, 3))
    run = np.repeat(np.arange(n), rng.integers(1, 5, n))[:n]
    if n > 250:
        run[250:261] = run[250]
    r["acc"][:, 2], r["gyr"][:, 2] = r["acc"][run, 2], r["gyr"][run, 2]
    ids = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(0, 41, n)]
    buf, off = synth.imu_messages(r, ids, seq0=seed, seed=seed)
    return r, buf, off


# ------------------------------------------------------------------ CPU: serialiser, reader, the restatement's rules
def test_serialiser_and_reader_round_trip_at_every_frame_id_residue():
    rng = np.random.default_rng(1)
    n = 41
    r = np.zeros(n, dtype=synth.IMU_DTYPE)
    r["stamp"] = 1234.0 + np.arange(n) * 0.125   # exact in sec / nsec
    r["acc"], r["gyr"] = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    ids = [b"x" * k for k in range(n)]           # lengths 0 .. 40: every residue mod 8
    buf, off = synth.imu_messages(r, ids, seq0=9)
    assert list(np.diff(off.astype(np.int64))) == [abi.LK_IMU_MSG_FIXED_BYTES + k for k in range(n)] and off[-1] == len(buf)
    m = imu_ref.read_imu_messages(buf, off)
    assert list(m["seq"]) == list(range(9, 9 + n)) and [f for f in m["frame_id"]] == ids
    assert np.array_equal(m["acc"], r["acc"]) and np.array_equal(m["gyr"], r["gyr"])
    assert np.array_equal(m["sec"] + 1e-9 * m["nsec"], r["stamp"])
    out = imu_ref.Frontend(False).process(buf, off)
    assert out.tobytes() == r.tobytes()
    # a stamp that is no multiple of a nanosecond decodes to toSec of its sec / nsec, not to the generator's double
    r2 = r[:1].copy()
    r2["stamp"] = 1.1
    got = imu_ref.Frontend(False).process(*synth.imu_messages(r2, b"imu"))
    assert got["stamp"][0] == 1.0 + 1e-9 * 100000000.0
    # bytes the decoder does not read are random (no test passes on zeros)
    assert (buf[int(off[5]) + 16 + 5 + 32:int(off[5]) + 16 + 5 + 100] != 0).mean() > 0.9
    with pytest.raises(imu_ref.BadLength):
        imu_ref.read_imu_messages(buf, np.r_[off[:-1], off[-1] - 1])


def test_redundancy_dropped_message_still_becomes_previous_and_zero_first_message_is_dropped():
    rows = [(0.0, 0.0),    # equals the zero-initialised static: dropped
            (1.0, 2.0),    # kept
            (1.0, 2.0),    # same as previous: dropped
            (1.0, 3.0),    # gyr differs: kept
            (5.0, 3.0),    # acc differs: kept
            (1.0, 2.0),    # equals messages 1 and 2, but previous is message 4: kept
            (1.0, 2.0)]    # equals message 5: dropped
    r = _imus(rows)
    fe = imu_ref.Frontend(True)
    out = fe.process(*synth.imu_messages(r, "imu_link"))
    assert list(np.round((out["stamp"] - 7.0) / 0.005).astype(int)) == [1, 3, 4, 5]
    assert fe.last_acc_z == 1.0 and fe.last_gyr_z == 2.0   # the previous message is the last one given, dropped or not
    assert fe.process(*synth.imu_messages(_imus([(1.0, 2.0)], t0=8.0), "imu_link")).size == 0
    assert imu_ref.Frontend(False).process(*synth.imu_messages(r, "imu_link")).size == len(rows)


def test_redundancy_signed_zero_matches_and_nan_never_does():
    fe = imu_ref.Frontend(True)
    out = fe.process(*synth.imu_messages(_imus([(-0.0, 0.0),             # -0 == +0: equals the zero static -> dropped
                                                (float("nan"), 1.0),      # kept
                                                (float("nan"), 1.0)]), ""))   # NaN != NaN -> kept
    assert out.size == 2


def test_backwards_stamp_raises_and_keeps_the_state():
    fe = imu_ref.Frontend(False)
    fe.process(*synth.imu_messages(_imus([(1.0, 1.0)], t0=5.0), "a"))
    before = fe.state()
    r = _imus([(2.0, 2.0), (3.0, 3.0)], t0=6.0)
    r["stamp"][1] = 4.0
    with pytest.raises(imu_ref.BackwardsStamp):
        fe.process(*synth.imu_messages(r, "a"))
    assert fe.state() == before


def test_imu_frontend_state_size_matches_a_c_compiler(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "legkilo_hip.h"\nint main(void){printf("%zu %zu %zu %d\\n", '
                   'sizeof(lk_imu_frontend_state), offsetof(lk_imu_frontend_state, last_gyr_z), offsetof(lk_imu_frontend_state, last_stamp), '
                   'LK_IMU_MSG_FIXED_BYTES);return 0;}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [24, abi.lk_imu_frontend_state.last_gyr_z.offset, abi.lk_imu_frontend_state.last_stamp.offset, abi.LK_IMU_MSG_FIXED_BYTES]
    assert C.sizeof(abi.lk_imu_frontend_state) == 24 and abi.LK_IMU_MSG_FIXED_BYTES == synth.IMU_MSG_FIXED_BYTES == 312


def test_imu_start_host_mirror_compiles(tmp_path):
    from legkilo_amd import binding

    binding.build()
    src = os.path.join(ROOT, "leg-kilo_amd", "host", "example_imu_start.cc")
    exe = str(tmp_path / "lk_imu_start_example")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "leg-kilo_amd", "host"),
                        src, "-o", exe, "-L", os.path.join(ROOT, "leg-kilo_amd"), "-llegkilo_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "leg-kilo_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ------------------------------------------------------------------ GPU
def _handle(hip_lib, params, n_slots=1):
    return hip_lib.LegKiloHip(config.make_config(params, n_slots=n_slots, **SMALL))


def _decode_dev(g, buf, off):
    """buf -> HBM, lk_decode_imu_dev, the kept records back."""
    d_in, d_out = g.device_malloc(max(buf.nbytes, 1)), g.device_malloc(max(len(off) - 1, 1) * REC)
    try:
        g.h2d(d_in, buf)
        k = g.decode_imu_dev(d_in, off, d_out)
        out = np.zeros(k, dtype=synth.IMU_DTYPE)
        if k:
            g.d2h(out, d_out)
    finally:
        g.device_free(d_in)
        g.device_free(d_out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("redundancy", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_decode_parity_with_the_restatement(hip_lib, n, redundancy):
    _, buf, off = _stream(n, seed=40 + n)
    fe = imu_ref.Frontend(redundancy)
    ref = fe.process(buf, off)
    g = _handle(hip_lib, _params(redundancy))
    try:
        g.imu_configure(redundancy)
        out = _decode_dev(g, buf, off)
        st = g.imu_get_frontend()
    finally:
        g.close()
    assert out.tobytes() == ref.tobytes()   # integer -> double conversions and copies only: bit-equal
    assert st == fe.state()
    if not redundancy:
        assert len(out) == n
    elif n >= 63:
        assert 0 < len(out) < n and n - len(out) > n // 4   # the holds are dropped, their first messages kept
    else:
        assert len(out) == 1


@pytest.mark.gpu
def test_host_equals_device_and_chunks_equal_one_call(hip_lib):
    n = 5000
    _, body, off0 = _stream(n, seed=9)
    buf = np.r_[np.array([0xAB, 0xCD, 0xEF], dtype=np.uint8), body]   # msg_off[0] = 3
    off = off0 + np.uint64(3)
    g = _handle(hip_lib, _params(True))
    try:
        g.imu_configure(True)
        host = g.decode_imu(buf, off)
        st_host = g.imu_get_frontend()
        g.imu_configure(True)
        d_in, d_out = g.device_malloc(buf.nbytes + 1), g.device_malloc(n * REC)
        g.h2d(d_in + 1, buf)   # the device pointer and msg_off[0] at odd byte offsets
        k = g.decode_imu_dev(d_in + 1, off, d_out)
        dev = np.zeros(k, dtype=synth.IMU_DTYPE)
        g.d2h(dev, d_out)
        st_dev = g.imu_get_frontend()
        # 7 uneven chunks, one of them a single message
        g.imu_configure(True)
        cuts = [0, 1, 2, 97, 1001, 1002, 3333, n]
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            kk = g.decode_imu_dev(d_in + 1, off[a:b + 1], d_out)
            part = np.zeros(kk, dtype=synth.IMU_DTYPE)
            if kk:
                g.d2h(part, d_out)
            parts.append(part)
        st_chunks = g.imu_get_frontend()
        g.device_free(d_in)
        g.device_free(d_out)
    finally:
        g.close()
    fe = imu_ref.Frontend(True)
    ref = fe.process(buf, off)
    assert 0 < len(ref) < n
    assert host.tobytes() == ref.tobytes() and dev.tobytes() == host.tobytes() and np.concatenate(parts).tobytes() == host.tobytes()
    assert st_host == st_dev == st_chunks == fe.state()


@pytest.mark.gpu
def test_refusals_leave_the_state_alone(hip_lib):
    n = 400
    r, buf, off = _stream(n, seed=13)
    g = _handle(hip_lib, _params(False))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    try:
        out = np.zeros(n, dtype=synth.IMU_DTYPE)
        cnt = C.c_size_t()
        assert g.L.lk_decode_imu(g.h, vp(buf), C.c_size_t(n), vp(off), None, C.byref(cnt)) == -1                  # null output
        assert g.L.lk_decode_imu(g.h, vp(buf), C.c_size_t(n), vp(off), vp(out), C.byref(cnt)) == -5               # LK_ERR_STATE: never configured
        assert g.L.lk_imu_get_frontend(g.h, C.byref(abi.lk_imu_frontend_state())) == -5
        g.imu_configure(False)
        assert g.L.lk_decode_imu(g.h, vp(buf), C.c_size_t(0), vp(off), vp(out), C.byref(cnt)) == 0 and cnt.value == 0   # n == 0
        first = g.decode_imu(buf, off[:101])
        before = g.imu_get_frontend()

        def refused(b, o, match):
            with pytest.raises(hip_lib.LegKiloError, match=r"error -1: .*" + match):
                g.decode_imu(b, o)
            d = g.device_malloc(len(b))
            try:
                g.h2d(d, b)
                with pytest.raises(hip_lib.LegKiloError, match=r"error -1: .*" + match):
                    g.decode_imu_dev(d, o, d_scr)
            finally:
                g.device_free(d)
            assert g.imu_get_frontend() == before

        d_scr = g.device_malloc(n * REC)
        rest, o_rest = buf[int(off[100]):].copy(), off[100:] - off[100]
        # a message shorter than the fixed part; a decreasing msg_off
        short = o_rest[:7].copy()
        short[6] = short[5] + np.uint64(311)
        refused(rest, short, "message 5: shorter")
        bad = o_rest.copy()
        bad[7] = bad[5]
        refused(rest, bad, "message 6: msg_off decreases")
        # a length that is not 312 + L (found on the device): message j, with a frame_id, loses its last byte to message j + 1
        j = 10 + int(np.flatnonzero(np.diff(o_rest[10:].astype(np.int64)) > 312)[0])
        bad = o_rest.copy()
        bad[j + 1] -= np.uint64(1)
        refused(rest, bad, f"message {j}: its length of ")
        # L = 0xFFFFFFFF in the LAST message of the buffer
        b2 = rest.copy()
        b2[int(o_rest[-2]) + 12:int(o_rest[-2]) + 16] = 0xFF
        refused(b2, o_rest, f"message {len(o_rest) - 2}: its length of ")
        # a stamp going backwards inside a call, and across calls
        r2 = r[100:].copy()
        r2["stamp"][50] -= 1.0
        ids = [bytes(m) for m in imu_ref.read_imu_messages(buf, off)["frame_id"][100:]]
        refused(*synth.imu_messages(r2, ids), "stamps go backwards")
        refused(buf[int(off[50]):int(off[60])].copy(), off[50:61] - off[50], "stamps go backwards")
        g.device_free(d_scr)
        # null pointers of the other entries
        a, b = C.c_size_t(), C.c_size_t()
        ends, nm = np.array([1.0, 2.0]), np.zeros(2, dtype=np.uint32)
        assert g.L.lk_imu_split_dev(g.h, None, C.c_size_t(4), vp(ends), C.c_size_t(2), vp(nm), C.byref(a), C.byref(b)) == -1
        assert g.L.lk_decode_imu_dev(g.h, None, C.c_size_t(4), vp(off), vp(out), C.byref(a)) == -1
        assert g.L.lk_imu_set_frontend(g.h, None) == -1
        # the stream goes on where it was
        more = g.decode_imu(buf, off[100:])
        fe = imu_ref.Frontend(False)
        assert first.tobytes() == fe.process(buf, off[:101]).tobytes() and more.tobytes() == fe.process(buf, off[100:]).tobytes()
        assert g.imu_get_frontend() == fe.state()
    finally:
        g.close()


@pytest.mark.gpu
def test_split_parity_with_stamps_on_scan_ends(hip_lib):
    """The arrays of test_kin_frontend.py::test_split_parity_with_stamps_on_scan_ends on lk_imu records; the same stamps as lk_kin_imu
    records through lk_kin_split_dev give the same table."""
    rng = np.random.default_rng(3)
    t = 2.0 + np.cumsum(rng.choice([0.002, 0.004, 0.02], 3000, p=[0.6, 0.3, 0.1]))
    t[100] = t[99]                   # two records at the same stamp
    t[500] = t[501] = t[499]         # three
    ends = np.sort(np.r_[t[rng.choice(len(t), 300, replace=False)], t[99], t[499], t[499], t[1000], t[1000],
                         rng.uniform(t[0] - 0.01, t[-1], 300), t[-1] + 0.001])
    imus, kins = np.zeros(len(t), dtype=synth.IMU_DTYPE), np.zeros(len(t), dtype=synth.KIN_DTYPE)
    imus["stamp"], kins["time_stamp"] = t, t
    imus["acc"] = rng.normal(size=(len(t), 3))
    g = _handle(hip_lib, _params(True))
    try:
        d = g.device_malloc(kins.nbytes)
        g.h2d(d, imus)
        n_msg, npk, ncs = g.imu_split_dev(d, len(imus), ends)
        g.h2d(d, kins)
        k_msg, kpk, kcs = g.kin_split_dev(d, len(kins), ends)
        g.device_free(d)
    finally:
        g.close()
    want = kin_ref.sync_package(t, ends)
    assert (npk, ncs) == (want[1], want[2]) and npk == len(ends) - 1
    assert np.array_equal(n_msg, want[0]) and (n_msg == 0).sum() > 10
    assert (kpk, kcs) == (npk, ncs) and np.array_equal(k_msg, n_msg)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 257])
def test_guard_bands_around_the_records(hip_lib, n):
    import devguard

    _, buf, off = _stream(n, seed=70 + n)
    ref = imu_ref.Frontend(True).process(buf, off)
    g = _handle(hip_lib, _params(True))
    try:
        g.imu_configure(True)
        d_in = devguard.Guarded.input(g, buf, offset=1, name=f"imu_msgs{n}")
        d_out = devguard.Guarded(g, n * REC, offset=8, name=f"imu_out{n}")
        k = g.decode_imu_dev(d_in.ptr, off, d_out.ptr)
        d_in.check()
        got = d_out.read(synth.IMU_DTYPE, k)
        assert got.tobytes() == ref.tobytes()
        devguard.untouched(d_out.check()[k * REC:])   # nothing behind the kept records
        d_imus = devguard.Guarded.input(g, ref if len(ref) else np.zeros(1, dtype=synth.IMU_DTYPE), offset=8, name=f"imu_recs{n}")
        ends = np.r_[ref["stamp"][::7], ref["stamp"][-1]]
        n_msg, npk, ncs = g.imu_split_dev(d_imus.ptr, len(ref), ends)
        d_imus.check()
        want = kin_ref.sync_package(ref["stamp"], ends)
        assert np.array_equal(n_msg, want[0]) and (npk, ncs) == (want[1], want[2])
        for b in (d_in, d_out, d_imus):
            b.free()
    finally:
        g.close()


@pytest.mark.gpu
def test_scratch_grows_and_stays_right(hip_lib):
    """A short stream, a long one, the short one again on one handle (lk_decode_imu_dev, then lk_imu_split_dev over what it kept, with few and
    with many scans): records, front-end state and split equal, bit for bit, what the same input gives on a fresh handle."""
    short, long_ = _stream(300, seed=31)[1:], _stream(20_000, seed=32)[1:]

    def run(g, buf, off, n_scans):
        g.imu_configure(True)   # (resets the carried state: every input starts like a first call)
        d_in, d_out = g.device_malloc(buf.nbytes), g.device_malloc((len(off) - 1) * REC)
        try:
            g.h2d(d_in, buf)
            k = g.decode_imu_dev(d_in, off, d_out)
            recs = np.zeros(k, dtype=synth.IMU_DTYPE)
            g.d2h(recs, d_out)
            st = g.imu_get_frontend()
            ends = np.linspace(recs["stamp"][0], recs["stamp"][-1] + 0.01, n_scans)
            n_msg, npk, ncs = g.imu_split_dev(d_out, k, ends)
        finally:
            g.device_free(d_in)
            g.device_free(d_out)
        assert k > 20 and npk > 0 and ncs > 0
        return recs.tobytes(), st, n_msg.tobytes(), npk, ncs

    one = _handle(hip_lib, _params(True))
    try:
        for (buf, off), n_scans in ((short, 3), (long_, 2500), (short, 3)):
            fresh = _handle(hip_lib, _params(True))
            try:
                want = run(fresh, buf, off, n_scans)
            finally:
                fresh.close()
            assert run(one, buf, off, n_scans) == want
    finally:
        one.close()


class _Standing:
    """A robot standing still at the trajectory's pose at t0: what a run starts from (the first frame takes gravity from the mean specific force)."""

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
def test_imu_mode_recorded_run_from_message_bytes(oracle_lib, hip_lib):
    """PointCloud2 + Imu bytes -> lk_decode_scan_dev (first cloud) / lk_decode_scans_dev (the others) / lk_decode_imu_dev -> lk_imu_split_dev over
    all 7 scan ends -> package 0: lk_first_frame_dev, packages 1 .. 6: lk_batch_replay_scans_imu_dev from the first-frame state - neither points
    nor records leave HBM.  Equals the oracle's first_frame + process_scan (insert off, each scan from the same prior) fed with the
    restatement's records (counts exact, x to 1e-8, P to 1e-6), and lk_batch_replay_scans_dev(msg_kind 1) fed with the same records from
    the host, bit for bit."""
    import preprocess_oracle as po
    import scenes

    P = dict(_params(True), lidar_type=1, time_scale=1.0, filter_num=3, blind=1.5, voxel_grid_resolution=0.3)
    sc = scenes.Scene(params=P, **CAPS)
    t0, S = 2.0, 6
    still = _Standing(sc.traj, t0)
    stamps = [t0 + 0.1 * s for s in range(S + 1)]
    msgs = [synth.cloud_message(synth.vlp16_scan(sc.world, still, tb, P, seed_noise=3083 + s), 1, tb, seed=s) for s, tb in enumerate(stamps)]
    buf, msg_off, n_points = synth.pack_cloud_run(msgs, seed=5)
    raw0, _, end0 = po.decode_vec(msgs[0], 1, 1.0, P["filter_num"], P["blind"], header_stamp=stamps[0])
    ref_scans, ref_tb, ref_te = [], [], [end0]
    for s in range(1, S + 1):
        dec, b, e = po.decode_vec(msgs[s], 1, 1.0, P["filter_num"], P["blind"], header_stamp=stamps[s])
        ref_scans.append(po.preprocess(dec, P["voxel_grid_resolution"]))
        ref_tb.append(b), ref_te.append(e)
    imus = synth.imu_stream(still, t0, ref_te[-1] + 0.02, seed=8600)
    imus["acc"][1::3, 2], imus["gyr"][1::3, 2] = imus["acc"][0::3, 2][:len(imus[1::3])], imus["gyr"][0::3, 2][:len(imus[1::3])]   # every third message repeats its z values
    rng = np.random.default_rng(6)
    ibuf, ioff = synth.imu_messages(imus, [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(0, 41, len(imus))], seed=8)
    ref = imu_ref.Frontend(True).process(ibuf, ioff)
    n_ref, npk, ncs = kin_ref.sync_package(ref["stamp"], ref_te)
    assert npk == S + 1 and min(n_ref) > 5 and len(ref) < len(imus)
    off = np.r_[0, np.cumsum(n_ref)]

    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    o.first_frame(raw0, end0, imus=ref[:off[1]])
    o.set_map_insert(False)
    x_ff, P_ff = o.get_state()
    g = hip_lib.LegKiloHip(sc.cfg(n_slots=S))
    dptrs = []
    try:
        g.imu_configure(P)
        total, PT = int(n_points.sum()), synth.POINT_DTYPE.itemsize
        dptrs = [g.device_malloc(nb) for nb in (buf.nbytes, int(n_points[0]) * PT, total * PT, ibuf.nbytes, len(imus) * REC)]
        d_bag, d_raw, d_pts, d_ibag, d_imus = dptrs
        g.h2d(d_bag, buf)
        g.h2d(d_ibag, ibuf)
        lay = synth.cloud_layout(1)
        n_raw, _, te0 = g.decode_scan_dev(d_bag + int(msg_off[0]), int(n_points[0]), lay, 1.0, P["filter_num"], P["blind"], stamps[0], d_raw)
        so, tb, te = g.decode_scans_dev(d_bag, msg_off[1:], n_points[1:], stamps[1:], lay, 1.0, P["filter_num"], P["blind"], P["voxel_grid_resolution"], d_pts)
        k = g.decode_imu_dev(d_ibag, ioff, d_imus)
        n_msg, n_pk, n_cs = g.imu_split_dev(d_imus, k, np.r_[te0, te])
        assert (n_raw, te0) == (len(raw0), end0) and list(tb) == ref_tb and list(te) == ref_te[1:]
        assert (k, n_pk, n_cs) == (len(ref), npk, ncs) and np.array_equal(n_msg, n_ref)
        g.first_frame_dev(d_raw, n_raw, te0, 1, d_imus, int(n_msg[0]))
        xg, Pg = g.get_state()
        assert np.array_equal(xg, x_ff) and np.array_equal(Pg, P_ff) and np.array_equal(g.get_Q(), o.get_Q())
        assert np.isclose(g.get_acc_norm(), o.get_acc_norm(), rtol=1e-15) and g.get_times() == o.get_times() == (end0, end0)
        scenes.compare_maps(o.map_export(), g.map_export())
        g.batch_set_priors(np.tile(xg, (S, 1)), np.tile(Pg.reshape(1, 900), (S, 1)))
        ps = g.batch_replay_scans_imu_dev(d_pts, so, tb, n_msg[1:], d_imus + int(n_msg[0]) * REC)
        dev_states = [g.get_state(slot=s) for s in range(S)]
        # the same records through the host
        recs = np.zeros(n_cs, dtype=synth.IMU_DTYPE)
        g.d2h(recs, d_imus)
        assert recs.tobytes() == ref[:n_cs].tobytes()
        per = np.split(recs, off[1:-1])
        g.batch_set_priors(np.tile(xg, (S, 1)), np.tile(Pg.reshape(1, 900), (S, 1)))
        ph = g.batch_replay_scans_dev(d_pts, so, tb, imus=per[1:])
        host_states = [g.get_state(slot=s) for s in range(S)]
        for s in range(S):
            assert bytes(ps[s]) == bytes(ph[s]), s
            assert dev_states[s][0].tobytes() == host_states[s][0].tobytes() and dev_states[s][1].tobytes() == host_states[s][1].tobytes(), s
            o.set_state(x_ff, P_ff)
            o.set_times(ref_tb[s], ref_tb[s])
            po_, _ = o.process_scan(ref_scans[s], ref_tb[s], imus=ref[off[s + 1]:off[s + 2]])
            xo, Po = o.get_state()
            xs, Ps = dev_states[s]
            assert (po_.n_buckets, po_.n_updates, po_.n_effect) == (ps[s].n_buckets, ps[s].n_updates, ps[s].n_effect), s
            assert po_.n_effect > 500, (s, po_.n_effect)
            assert np.allclose(xo, xs, rtol=1e-8, atol=1e-9), (s, np.abs(xo - xs).max())
            assert np.allclose(Po, Ps, rtol=1e-6, atol=1e-11), (s, np.abs(Po - Ps).max())
    finally:
        for d in dptrs:
            g.device_free(d)
        g.close()
        o.close()
