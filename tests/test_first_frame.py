"""The first frame of a run in one call (lk_first_frame(_dev): KILO.cc:332-352 - state initialisation from the first package's messages,
cloudLidarToWorld on the raw cloud, BuildVoxelMap, acc_norm_ and the time stamps), with the oracle's first_frame as checker and the
hand-composed start the rest of the suite uses (lk_set_state + lk_init_process_cov_q + lk_map_build on host-computed world points)."""
import ctypes as C
import functools

import numpy as np
import pytest

import offconfig
import scenes
from legkilo_amd import synth

CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)   # test_kin_frontend.py's
T0 = 2.0


@functools.lru_cache(maxsize=None)
def _inputs(name, use_kin):
    """(scene, raw first cloud, 37 messages of the package) of a configuration; computed once, never modified."""
    sc = offconfig.scene(name, use_kin, **CAPS)
    raw = synth.vlp16_scan(sc.world, scenes.Frozen(sc.traj, T0), T0, sc.P)
    if use_kin:
        msgs = synth.kin_stream(sc.traj, T0 - 0.1, T0, sc.P, seed=77)[:37]
    else:
        msgs = synth.imu_stream(sc.traj, T0 - 0.2, T0, seed=77)[:37]
    assert len(msgs) == 37
    raw.setflags(write=False), msgs.setflags(write=False)
    return sc, raw, msgs


def _same_map(a, b):
    """The same map bit for bit; node ids may differ between two builds (root voxels are created by racing threads)."""
    return np.array_equal(a, b) or scenes.maps_identical(a, b)


def _first_frame_dev(g, raw, end_time, msgs, kind):
    d_raw, d_msgs = g.device_malloc(raw.nbytes), g.device_malloc(msgs.nbytes)
    try:
        g.h2d(d_raw, raw)
        g.h2d(d_msgs, msgs)
        g.first_frame_dev(d_raw, len(raw), end_time, kind, d_msgs, len(msgs))
    finally:
        g.device_free(d_raw)
        g.device_free(d_msgs)


def _snapshot(g):
    x, P = g.get_state()
    return x.tobytes(), P.tobytes(), g.get_Q().tobytes(), g.get_acc_norm(), g.get_times()


@pytest.mark.gpu
@pytest.mark.parametrize("n_msg", [1, 2, 37])
@pytest.mark.parametrize("use_kin", [False, True])
@pytest.mark.parametrize("name", [None, "tilt"])
def test_first_frame_parity_with_the_oracle(oracle_lib, hip_lib, name, use_kin, n_msg):
    """At n_msg = 1 the first message is visited twice and the divisor is 1.  Every operation of the state chain is a correctly rounded fp64
    + - * / sqrt in the oracle's order: the state is compared for equality."""
    sc, raw, msgs = _inputs(name, use_kin)
    msgs = np.ascontiguousarray(msgs[:n_msg])
    kw = dict(kins=msgs) if use_kin else dict(imus=msgs)
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=not use_kin)
    g, gh = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    try:
        g.set_acc_norm(1.25)   # (overwritten by the call)
        o.first_frame(raw, T0, **kw)
        _first_frame_dev(g, raw, T0, msgs, 2 if use_kin else 1)
        gh.first_frame(raw, T0, **kw)
        (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
        print(f"{name} use_kin={use_kin} n_msg={n_msg}: max |x| diff {np.abs(xo - xg).max():.3g}, acc_norm {g.get_acc_norm()!r} vs {o.get_acc_norm()!r}")
        assert np.array_equal(xg, xo), np.abs(xo - xg).max()
        assert np.array_equal(xg[:9], np.eye(3).reshape(9)) and np.all(xg[9:18] == 0) and np.all(xg[24:] == 0) and abs(np.linalg.norm(xg[21:24]) - 9.81) < 1e-12
        assert np.array_equal(Pg, Po) and np.array_equal(Pg, 1e-6 * np.eye(30)) and np.array_equal(g.get_Q(), o.get_Q())
        assert np.isclose(g.get_acc_norm(), o.get_acc_norm(), rtol=1e-15) and g.get_times() == o.get_times() == (T0, T0)
        st = scenes.compare_maps(o.map_export(), g.map_export())
        assert st["roots"] > 500
        # the host entry: bit-equal to the device entry
        assert _snapshot(gh) == _snapshot(g)
        assert _same_map(gh.map_export(), g.map_export())
    finally:
        g.close()
        gh.close()
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [None, "tilt"])
def test_first_frame_equals_the_composed_start(hip_lib, name):
    """lk_first_frame == lk_set_state with the same numbers + lk_init_process_cov_q + lk_set_acc_norm + lk_set_times + lk_map_build on
    world points computed on the host by cloudLidarToWorld's plain products and sums: state and map bit for bit."""
    sc, raw, msgs = _inputs(name, False)
    g, c = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    try:
        g.first_frame(raw, T0, imus=msgs)
        x, P = g.get_state()
        c.set_state(x, P)
        c.init_process_cov_q()
        c.set_acc_norm(g.get_acc_norm())
        c.set_times(T0, T0)
        E, T = np.array(sc.P["extrinsic_R"], float).reshape(3, 3), np.array(sc.P["extrinsic_T"], float)
        R, p = x[:9].reshape(3, 3), x[9:12]
        l = [raw[f].astype(np.float64) for f in ("x", "y", "z")]
        b = [(E[r, 0] * l[0] + E[r, 1] * l[1] + E[r, 2] * l[2]) + T[r] for r in range(3)]
        w = np.stack([(R[r, 0] * b[0] + R[r, 1] * b[1] + R[r, 2] * b[2]) + p[r] for r in range(3)], axis=1).astype(np.float32)
        c.map_build(w, scenes.xyz_of(raw))
        assert _snapshot(c) == _snapshot(g)
        assert _same_map(c.map_export(), g.map_export())
    finally:
        g.close()
        c.close()


@pytest.mark.gpu
def test_first_frame_refusals_change_nothing(hip_lib):
    sc, raw, msgs = _inputs(None, False)
    g = hip_lib.LegKiloHip(sc.cfg(max_scan_points=1 << 15))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    try:
        g.set_state(np.arange(36.0), 2e-3 * np.eye(30))
        g.set_times(0.5, 0.75)
        g.set_acc_norm(3.5)
        before = _snapshot(g)
        d_raw, d_msgs = g.device_malloc(raw.nbytes), g.device_malloc(msgs.nbytes)
        g.h2d(d_raw, raw)
        g.h2d(d_msgs, msgs)

        def both(n, kind, n_msg):
            return (g.L.lk_first_frame(g.h, vp(raw), C.c_size_t(n), C.c_double(T0), C.c_int(kind), vp(msgs), C.c_size_t(n_msg)),
                    g.L.lk_first_frame_dev(g.h, C.c_void_p(d_raw), C.c_size_t(n), C.c_double(T0), C.c_int(kind), C.c_void_p(d_msgs), C.c_size_t(n_msg)))

        n = len(raw)
        for args, rc in (((n, 1, 0), -1),            # n_msg == 0: "Data packet is not ready"
                         ((0, 1, 37), -1),           # n == 0
                         ((n, 0, 37), -1),           # msg_kind 0
                         ((n, 3, 37), -1),           # msg_kind 3
                         (((1 << 15) + 1, 1, 37), -3)):   # n > max_scan_points: LK_ERR_CAPACITY
            if args[0] > n:
                big = np.zeros(args[0], dtype=synth.POINT_DTYPE)
                assert g.L.lk_first_frame(g.h, vp(big), C.c_size_t(len(big)), C.c_double(T0), C.c_int(1), vp(msgs), C.c_size_t(37)) == rc
            else:
                assert both(*args) == (rc, rc), args
            assert _snapshot(g) == before and g.map_stats() == (0, 0, 0), args
        # a second call on a built map: LK_ERR_STATE, state, times and map as the first call left them
        g.first_frame_dev(d_raw, n, T0, 1, d_msgs, 37)
        built, blob = _snapshot(g), g.map_export()
        assert built != before and g.map_stats()[0] > 500
        assert both(n, 1, 37) == (-5, -5)
        assert both(n, 1, 0) == (-1, -1)
        assert _snapshot(g) == built and np.array_equal(g.map_export(), blob)
        g.device_free(d_raw)
        g.device_free(d_msgs)
    finally:
        g.close()
