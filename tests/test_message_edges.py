"""-m gpu: every device code path that applies IMU / kinematic + IMU messages between time buckets, on the crafted streams of tests/msgcases.py -
all 16 contact masks (set bits written 1, 2, -1, 256), every second stamp exactly on a bucket time, a pair of equal stamps, the same at stamps of
1.7e9 s (consecutive buckets on one absolute time, dt = 0 predicts), and large buckets with a message on the next bucket's time - against the CPU
oracle, which tests/test_reference_pin.py pins against the reference's own KILO::process on these very streams.

  lk_update_imu / lk_update_kin_imu (lk_imu_kernel, lk_kin_kernel)       test_update_kin_imu_every_mask, test_launches_*, test_live_* (launches)
  run_scan_launches (lk_stream.hip)                                      test_live_scan_resident_and_launches, test_launches_with_large_buckets_and_messages
  lk_scan_stream_kernel<MSG>                                             test_live_scan_resident_and_launches
  dev_scan_wave (lk_batch_replay_ragged_* / _scans_*_dev)                test_frozen_replay_ragged
  lk_rag_advance_kernel                                                  test_overlay_ragged_resident_and_launches, test_overlay_runs (LEGKILO_RAG_RESIDENT=0)
  lk_rag_ov_scan_kernel, plain and RUN form                              test_overlay_ragged_resident_and_launches, test_overlay_runs
  the runs' advance in lk_overlay.hip                                    test_overlay_runs (LEGKILO_RAG_RESIDENT=0)

Tolerances are those of the existing test of the same entry (named at each assertion).  Every test asserts the conditions on its input
(msgcases.assert_conditions: masks, ties, equal bucket times, and that a tie or a mask changes the ORACLE's answer by 1e3 tolerances) before it
looks at a device result.  The oracle's runs are computed once per (kind, when) and shared.
"""
import numpy as np
import pytest

import msgcases as mc
import scenes
import test_overlay_runs as tor   # oracle_run, check_parity, pose_bits: the helpers and tolerances test_overlay_runs asks of the entry
from legkilo_amd import synth
from scenes import rand_spd, rel_err

pytestmark = pytest.mark.gpu

KINDS = ["kin", "imu"]
WHENS = ["t1", "epoch"]   # the size of the time stamps: seconds (the cases start at msgcases.T0 = 3 s), or the same + 1.7e9 s


def counts(p):
    return (p.n_buckets, p.n_updates, int(p.n_effect))


def kw(kind, msgs):
    return {"kins" if kind == "kin" else "imus": msgs}


def close(*objs):
    for obj in objs:
        obj.close()


# ----------------------------------------------------------------------------- the live path: scan-resident kernel and per-bucket launches
@pytest.mark.parametrize("when", WHENS)
@pytest.mark.parametrize("kind", KINDS)
def test_live_scan_resident_and_launches(oracle_lib, hip_lib, kind, when):
    """First frame + 4 scans with insert through lk_scan_stream_kernel<MSG> (default) and through run_scan_launches (lk_stream_resident(0): one
    lk_imu_kernel / lk_kin_kernel launch per message): the two bit-identical (state, covariance, re-projected cloud, map), both equal to the
    oracle - counts exact on every scan, state rtol 1e-7 / atol 1e-8 (kin, test_sequence_kin_mode) or 1e-7 (imu,
    test_scan_resident_kernel_equals_per_bucket_launches), both time stamps exactly, map as in sequence_scan_resident_and_launches."""
    c = mc.live_case(kind, when == "epoch")
    mc.assert_conditions(c, 1e-7)
    g, g_pb = hip_lib.LegKiloHip(c.sc.cfg()), hip_lib.LegKiloHip(c.sc.cfg())
    g_pb.stream_resident(False)
    for obj in (g, g_pb):
        mc.start(obj, c)
    for s, scan in enumerate(c.scans):
        cnt, xo, times = c.oracle[s]
        pg, wg = g.process_scan(scan["ds"], scan["tb"], want_world=True, **kw(kind, scan["msgs"]))
        pp, wp = g_pb.process_scan(scan["ds"], scan["tb"], want_world=True, **kw(kind, scan["msgs"]))
        (xg, Pg), (xp, Pp) = g.get_state(), g_pb.get_state()
        print(f"{kind} {when} scan {s}: counts {cnt} / {counts(pg)} / {counts(pp)}, max |dx| resident {np.abs(xo - xg).max():.2e}, launches {np.abs(xo - xp).max():.2e}")
        assert cnt == counts(pg) == counts(pp), (s, cnt, counts(pg), counts(pp))
        if kind == "kin":
            assert np.allclose(xo, xg, rtol=1e-7, atol=1e-8), (s, np.abs(xo - xg).max())
        else:
            assert np.abs(xo - xg).max() < 1e-7, (s, np.abs(xo - xg).max())
        assert g.get_times() == g_pb.get_times() == times, (s, g.get_times(), g_pb.get_times(), times)
        assert np.array_equal(xg, xp) and np.array_equal(Pg, Pp), (s, np.abs(xg - xp).max())
        assert np.array_equal(wg, wp), s
    scenes.maps_identical(g.map_export(), g_pb.map_export())
    scenes.compare_maps(c.oracle_map, g.map_export(), rtol=1e-5, ptol=1e-6)
    assert g.stream_resident_stats()[0] == len(c.scans) and g_pb.stream_resident_stats()[0] == 0
    close(g, g_pb)


# ----------------------------------------------------------------------------- one message at a time
@pytest.fixture()
def pair(oracle_lib, hip_lib):
    sc = mc.scene()
    o, g = oracle_lib.Oracle(sc.cfg(), imu_mode_only=False), hip_lib.LegKiloHip(sc.cfg())
    for obj in (o, g):
        obj.init_process_cov_q()
        obj.set_acc_norm(9.81)
    yield sc, o, g
    close(g, o)


def test_update_kin_imu_every_mask(pair):
    """lk_update_kin_imu (lk_kin_kernel: two predicts, the rows, the update) on one message per contact mask from a common prior: state and
    covariance as in test_update_by_imu_and_kin (rtol 1e-9 / atol 1e-11, relative 1e-9), both time stamps the message's."""
    sc, o, g = pair
    rng = np.random.default_rng(7)
    t = 1.0
    x0, P0 = synth.initial_state(sc.traj, t, sc.P), rand_spd(rng)
    x0[15:21] = rng.normal(0, 0.01, 6)
    kins = mc.one_message_per_mask(sc, t)
    assert set(mc.masks_of(kins)) == set(range(16)) and set(np.unique(kins["contact"])) == {0, 1, 2, -1, 256}
    for mask in range(16):
        g.set_state(x0, P0)
        g.set_times(t, t)
        o.set_state(x0, P0)
        o.set_times(t, t)
        o.update_kin_imu(kins[mask:mask + 1])
        g.update_kin_imu(kins[mask:mask + 1])
        (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
        assert np.abs(xo - x0).max() > 1e-6, mask
        assert np.allclose(xg, xo, rtol=1e-9, atol=1e-11), (mask, np.abs(xg - xo).max())
        assert rel_err(Pg, Po) < 1e-9, (mask, rel_err(Pg, Po))
        assert g.get_times() == o.get_times() == (kins["time_stamp"][mask],) * 2


def test_update_by_kin_imu_row_counts(pair):
    """The class surface lk_update_by_kin_imu at M = 6, 9, 12, 15, 18: the rows KILO.cc:267-309 builds for every contact mask (a contact's
    block at its rank among the feet in contact).  Tolerance of test_update_by_imu_and_kin."""
    sc, o, g = pair
    rng = np.random.default_rng(8)
    x0, P0 = synth.initial_state(sc.traj, 1.0, sc.P), rand_spd(rng)
    x0[15:21] = rng.normal(0, 0.01, 6)
    seen_m = set()
    for mask, rec in enumerate(mc.one_message_per_mask(sc, 1.0)):
        H, z, R = mc.kin_rows(x0, rec, sc.P)
        seen_m.add(len(z))
        for obj in (o, g):
            obj.set_state(x0, P0)
            obj.update_by_kin_imu(H, z, R)
        (xo, Po), (xg, Pg) = o.get_state(), g.get_state()
        assert np.abs(xo - x0).max() > 1e-6, mask
        assert np.allclose(xg, xo, rtol=1e-9, atol=1e-11), (mask, len(z), np.abs(xg - xo).max())
        assert rel_err(Pg, Po) < 1e-9, (mask, len(z), rel_err(Pg, Po))
    assert seen_m == {6, 9, 12, 15, 18}


# ----------------------------------------------------------------------------- large buckets: the predict that rides in the bucket before
@pytest.mark.parametrize("kind", KINDS)
def test_launches_with_large_buckets_and_messages(oracle_lib, hip_lib, kind):
    """run_scan_launches on four buckets of 600 points (all above LK_SMALL_MAX = 512: the next bucket's predict rides in a bucket's launch unless a
    message lies strictly before the next bucket's time) with no message before T2, one exactly on T2 and two strictly inside (T2, T3): bucket 1's and
    bucket 2's predicts ride - bucket 2's with the queue's head on its own time -, bucket 3's does not; the message on T2 is applied in front of
    bucket 3.  Counts exact, state rtol 1e-7 / atol 1e-8 (kin, test_sequence_kin_mode) or all 36 entries 1e-7 (imu,
    test_scan_resident_kernel_equals_per_bucket_launches), times exact; the pipelined form of the launches (lk_stream_pipeline(1)) bit-identical
    to the sequential one."""
    sc = mc.scene()
    ds, msgs = mc.dense_with_messages(sc, mc.T0, kind)
    T = mc.bucket_times(ds, mc.T0)
    st = msgs[mc.stamp_name(msgs)]
    sizes = np.diff(synth.buckets_of(ds)[0].astype(np.int64))
    assert sizes.min() > 512
    assert len(st) == 3 and st[0] == T[2] and T[2] < st[1] < st[2] < T[3]
    assert mc.rides(T, st, sizes) == [(True, T[2]), (True, T[2]), (False, T[2])]   # the host loop's decisions; at the second the head stamp IS the next bucket's time

    def oracle(m):
        o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=kind != "kin")
        x0 = scenes.init_filter(o, sc, mc.T0)
        scenes.first_frame(o, sc, mc.T0, x0)
        po, _ = o.process_scan(ds, mc.T0, **kw(kind, m))
        out = counts(po), o.get_state()[0].copy(), o.get_times()
        o.close()
        return out

    cnt, xo, times = oracle(msgs)
    assert cnt[0] == 4 and cnt[2] > 500
    # the message on T2 decides something: losing it, or popping it one bucket early (`<=`: one ulp down), moves the oracle's state by 1e3 tolerances
    lost = np.abs(oracle(msgs[1:])[1] - xo).max()
    early = np.abs(oracle(mc.ties_moved_down(msgs, T))[1] - xo).max()
    assert lost >= 1e3 * 1e-7 and early >= 1e3 * 1e-7, (lost, early)
    g, g_pipe = hip_lib.LegKiloHip(sc.cfg()), hip_lib.LegKiloHip(sc.cfg())
    g_pipe.stream_pipeline(True)   # off by default; the insert of bucket k beside predict, messages and residual pass of bucket k + 1
    for obj in (g, g_pipe):
        x0 = scenes.init_filter(obj, sc, mc.T0)
        scenes.first_frame(obj, sc, mc.T0, x0)
    pg, _ = g.process_scan(ds, mc.T0, **kw(kind, msgs))
    pq, _ = g_pipe.process_scan(ds, mc.T0, **kw(kind, msgs))
    (xg, Pg), (xq, Pq) = g.get_state(), g_pipe.get_state()
    print(f"large buckets {kind}: counts {cnt} / {counts(pg)}, max |dx| {np.abs(xo - xg).max():.2e}; the oracle moves {lost:.2e} without the message on T2, {early:.2e} with it one ulp early")
    assert counts(pg) == cnt
    if kind == "kin":
        assert np.allclose(xo, xg, rtol=1e-7, atol=1e-8), np.abs(xo - xg).max()
    else:
        assert np.abs(xo - xg).max() < 1e-7, np.abs(xo - xg).max()
    assert g.get_times() == times
    assert g.stream_resident_stats()[0] == 0, "a scan of large buckets with messages takes the per-bucket launches"
    # the pipelined form of the same launches: the same bits (as test_stream_pipeline_forced_conflicts asserts without messages)
    assert counts(pq) == cnt and np.array_equal(xg, xq) and np.array_equal(Pg, Pq), np.abs(xg - xq).max()
    scenes.maps_identical(g.map_export(), g_pipe.map_export())
    assert g_pipe.stream_stats()[0] == 4 and g.stream_stats()[0] == 0, (g_pipe.stream_stats(), g.stream_stats())
    close(g, g_pipe)


# ----------------------------------------------------------------------------- frozen-map replay: dev_scan_wave
def replay_handle(hip_lib, c):
    g = hip_lib.LegKiloHip(c.sc.cfg(n_slots=len(c.scans)))
    g.map_import(c.blob)
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    return g


def replay_args(c):
    return [s["ds"] for s in c.scans], [s["tb"] for s in c.scans], [s["msgs"] for s in c.scans]


@pytest.mark.parametrize("when", WHENS)
@pytest.mark.parametrize("kind", KINDS)
def test_frozen_replay_ragged(oracle_lib, hip_lib, kind, when):
    """lk_batch_replay_ragged_imu/_kin_dev (host-built tables) and lk_batch_replay_scans_dev (device-built) on 4 scans with perturbed priors over
    a frozen mature map, as test_batch_replay_ragged_leg_fusion: counts exact, x rtol 1e-8 / atol 1e-9, P rtol 1e-6 / atol 1e-11, the two
    table builds bit-identical."""
    c = mc.replay_case(kind, when == "epoch")
    mc.assert_conditions(c, 1e-8)
    scans, tbs, msgs = replay_args(c)
    Ps = [c.P0] * len(scans)
    g = replay_handle(hip_lib, c)
    ps = g.batch_replay_ragged(scans, tbs, c.xs, Ps, host_tables=True, **kw(kind, msgs))
    host_tab = [g.get_state(slot=s) for s in range(len(scans))]
    for s, (cnt, xo, Po) in enumerate(c.oracle_frozen):
        xg, Pg = host_tab[s]
        print(f"frozen {kind} {when} slot {s}: counts {cnt} / {counts(ps[s])}, max |dx| {np.abs(xo - xg).max():.2e}, max |dP| {np.abs(Po - Pg).max():.2e}")
        assert counts(ps[s]) == cnt, (s, cnt, counts(ps[s]))
        assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (s, np.abs(xo - xg).max())
        assert np.allclose(Po, Pg, rtol=1e-6, atol=1e-11), (s, np.abs(Po - Pg).max())
    pd = g.batch_replay_ragged(scans, tbs, c.xs, Ps, host_tables=False, **kw(kind, msgs))
    for s in range(len(scans)):
        assert counts(pd[s]) == counts(ps[s]), s
        xd, Pd = g.get_state(slot=s)
        assert np.array_equal(xd, host_tab[s][0]) and np.array_equal(Pd, host_tab[s][1]), s
    g.close()


# ----------------------------------------------------------------------------- replay with insert: scan-resident and launch by launch
@pytest.mark.parametrize("when", WHENS)
@pytest.mark.parametrize("kind", KINDS)
def test_overlay_ragged_resident_and_launches(oracle_lib, hip_lib, kind, when, monkeypatch):
    """lk_batch_replay_overlay_ragged_dev in its scan-resident form (lk_rag_ov_scan_kernel) and launch by launch (LEGKILO_RAG_RESIDENT=0:
    lk_rag_advance_kernel): per slot the oracle on a private copy of the map with insert on - counts, state 1e-6, covariance 1e-6 max|P|,
    private voxels, as in test_batch_replay_overlay_ragged -, the two forms bit-identical as in test_batch_replay_overlay_ragged_scan_resident."""
    c = mc.replay_case(kind, when == "epoch")
    mc.assert_conditions(c, 1e-6)
    want = mc.overlay_oracle(kind, when == "epoch")
    base = scenes.canon_map(c.blob)
    scans, tbs, msgs = replay_args(c)
    S = len(scans)
    Ps = [c.P0] * S
    g = replay_handle(hip_lib, c)
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
    poses = g.batch_replay_overlay_ragged(scans, tbs, c.xs, Ps, **kw(kind, msgs))
    assert g.overlay_resident_rounds() >= 1
    X, P = g.batch_get_states(0, S)
    exports = [g.overlay_export(s) for s in range(S)]
    for s, (cnt, xo, Po, omap) in enumerate(want):
        print(f"overlay {kind} {when} slot {s}: counts {cnt} / {counts(poses[s])}, max |dx| {np.abs(xo - X[s]).max():.2e}")
        assert counts(poses[s]) == cnt, (s, cnt, counts(poses[s]))
        assert np.abs(xo - X[s]).max() < 1e-6, (s, np.abs(xo - X[s]).max())
        assert np.abs(P[s] - Po).max() <= 1e-6 * np.abs(Po).max(), s
        st = scenes.compare_overlay(exports[s], base, omap, (kind, when, s), rtol=1e-5, ptol=1e-7)
        assert st["private_roots"] > 0 and st["changed_roots"] > 0, (s, st)
    monkeypatch.setenv("LEGKILO_RAG_RESIDENT", "0")
    poses0 = g.batch_replay_overlay_ragged(scans, tbs, c.xs, Ps, **kw(kind, msgs))
    assert g.overlay_resident_rounds() == 0
    X0, P0 = g.batch_get_states(0, S)
    assert np.array_equal(X, X0) and np.array_equal(P, P0), "scan-resident and launch-by-launch replay differ"
    for s in range(S):
        assert counts(poses0[s]) == counts(poses[s]), s
        assert scenes.maps_identical(g.overlay_export(s), exports[s]), s
    g.close()


# ----------------------------------------------------------------------------- whole runs with insert
@pytest.mark.parametrize("when", WHENS)
@pytest.mark.parametrize("kind", KINDS)
def test_overlay_runs(oracle_lib, hip_lib, kind, when, monkeypatch):
    """lk_batch_replay_overlay_runs_dev with 2 runs of 2 scans, run-resident (the RUN form of lk_rag_ov_scan_kernel) and launch by launch
    (LEGKILO_RAG_RESIDENT=0: the runs' advance on the CSR tables): the oracle scan after scan with the helpers and tolerances of
    tests/test_overlay_runs.py (check_parity), the two forms bit-identical (test_resident_equals_launch_by_launch)."""
    c = mc.replay_case(kind, when == "epoch")
    mc.assert_conditions(c, 1e-6)   # (the tolerance of a run's first scan)
    scans, tbs, msgs = replay_args(c)
    runs, tb_runs, msg_runs, xs = [scans[0:2], scans[2:4]], [tbs[0:2], tbs[2:4]], [msgs[0:2], msgs[2:4]], [c.xs[0], c.xs[2]]
    for r in range(2):
        assert tb_runs[r][0] + float(runs[r][0]["curvature"][-1]) < tb_runs[r][1]
    if when == "epoch":   # both runs' scan boundary lies between two pairs of buckets on one absolute time
        T = [s["T"] for s in c.scans]
        assert all(T[2 * r][-1] == T[2 * r][-2] and T[2 * r + 1][0] == T[2 * r + 1][1] for r in range(2))
    o = oracle_lib.Oracle(c.sc.cfg(), imu_mode_only=kind != "kin")
    o.init_process_cov_q()
    o.set_acc_norm(9.81)
    case = dict(mode=kind, runs=runs, base=scenes.canon_map(c.blob),
                oracle=[tor.oracle_run(o, c.blob, xs[r], c.P0, runs[r], tb_runs[r], kind, msg_runs[r]) for r in range(2)])
    o.close()
    g = hip_lib.LegKiloHip(c.sc.cfg(n_slots=2))
    g.map_import(c.blob)
    g.init_process_cov_q()
    g.set_acc_norm(9.81)
    monkeypatch.delenv("LEGKILO_RAG_RESIDENT", raising=False)
    poses = g.batch_replay_overlay_runs(runs, tb_runs, xs, [c.P0] * 2, **kw(kind, msg_runs))
    assert g.overlay_resident_rounds() >= 1
    X, P = g.batch_get_states(0, 2)
    exports = [g.overlay_export(r) for r in range(2)]
    tor.check_parity(case, poses, X, P, exports, f"{kind} {when}")
    monkeypatch.setenv("LEGKILO_RAG_RESIDENT", "0")
    poses0 = g.batch_replay_overlay_runs(runs, tb_runs, xs, [c.P0] * 2, **kw(kind, msg_runs))
    assert g.overlay_resident_rounds() == 0
    X0, P0 = g.batch_get_states(0, 2)
    assert np.array_equal(X, X0) and np.array_equal(P, P0), "run-resident and launch-by-launch replay differ"
    assert tor.pose_bits(poses0) == tor.pose_bits(poses)
    for r in range(2):
        assert scenes.maps_identical(g.overlay_export(r), exports[r]), r
    g.close()
