"""Pins the two scan-boundary rules that the batch replay of whole runs (lk_batch_replay_overlay_runs_dev) rests on, on the CPU, before any
device code is trusted.  KILO::process takes its package `measure` by value (KILO.cc:316-399): one call per scan, a new package every time.

  (i)  What scan k's package holds beyond that scan's last bucket time is DROPPED: it is not applied in front of scan k + 1.
  (ii) At scan k + 1's first bucket every record of ITS package below that bucket's time is applied - also one stamped before scan k's
       last bucket time; there is no look-back skip across the scan boundary.

The oracle's process_scan, called scan after scan, is compared with oracle/_ref's KILO::process (the drivers of test_reference_pin.py) on a
two-scan IMU-mode sequence and a two-scan kinematic sequence that carry both record kinds; then the oracle alone shows that the records of
(i) change nothing, bit for bit, and that the record of (ii) does.
"""
import numpy as np
import pytest

import oracle_binding as ob
import offconfig
import scenes
from legkilo_amd import synth

T0 = 1.0


def boundary_messages(sc, use_kin, scans, tbs, leftovers=True, lookback=True):
    """Per-scan packages of a two-scan sequence: the stream over [tb, tb + 0.1] up to the scan's last bucket time; scan 0's package then
    carries (i) three records stamped after its last bucket time and before scan 1's first bucket, scan 1's package (ii) one record stamped
    1 ms before scan 0's last bucket time."""
    stamp = "time_stamp" if use_kin else "stamp"
    out = []
    last0 = tbs[0] + float(scans[0]["curvature"][-1])
    first1 = tbs[1] + float(scans[1]["curvature"][0])
    assert last0 + 1.5e-3 < first1, (last0, first1)
    for k, (pts, tb) in enumerate(zip(scans, tbs)):
        m = synth.kin_stream(sc.traj, tb, tb + 0.1, sc.P, seed=3003 + k) if use_kin else synth.imu_stream(sc.traj, tb, tb + 0.1, seed=3003 + k)
        m = m[m[stamp] < tb + float(pts["curvature"][-1])]
        assert len(m) > 5
        if k == 0 and leftovers:
            extra = m[-3:].copy()
            extra[stamp] = last0 + (first1 - last0) * np.array([0.25, 0.5, 0.75])
            assert np.all(extra[stamp] > last0) and np.all(extra[stamp] < first1)
            m = np.concatenate([m, extra])
        if k == 1 and lookback:
            early = m[:1].copy()
            early[stamp] = last0 - 1e-3
            m = np.concatenate([early, m])
        assert np.all(np.diff(m[stamp]) > 0)
        out.append(m)
    return out


def two_scans(sc):
    tbs = [T0, T0 + 0.12]   # a scan spans 0.1 s: 20 ms between scan 0's last bucket and scan 1's first
    return [scenes.vlp_scan_input(sc, tb, k) for k, tb in enumerate(tbs)], tbs


def run(obj, sc, use_kin, scans, tbs, msgs):
    x0 = scenes.init_filter(obj, sc, T0)
    scenes.first_frame(obj, sc, T0, x0)
    out = []
    for pts, tb, m in zip(scans, tbs, msgs):
        pose, _ = obj.process_scan(pts, tb, **({"kins": m} if use_kin else {"imus": m}))
        x, P = obj.get_state()
        out.append((pose, x.copy(), P.copy()))
    return out


def bits(res, obj):
    return [(int(p.n_effect), p.n_buckets, p.n_updates, x.tobytes(), P.tobytes(), np.array(p.rot).tobytes(), np.array(p.pos).tobytes(),
             np.array(p.vel).tobytes()) for p, x, P in res] + [obj.get_times()]


@pytest.mark.skipif(ob.build_ref() is None, reason="oracle/_ref not built and the reference sources absent")
@pytest.mark.parametrize("use_kin", [False, True])
def test_process_scan_after_scan_matches_the_reference_at_the_boundary(tmp_path, use_kin):
    """Oracle against the reference's KILO::process, both called scan after scan with packages that carry (i) and (ii): match counts exact,
    states and covariance to test_reference_pin.py's tolerances."""
    sc = offconfig.scene(None, use_kin)
    o = ob.Oracle(sc.cfg(), imu_mode_only=not use_kin)
    k = ob.ReferenceKilo(sc.P, not use_kin, tmp_path / "ref.yaml")
    scans, tbs = two_scans(sc)
    msgs = boundary_messages(sc, use_kin, scans, tbs)
    ro, rk = run(o, sc, use_kin, scans, tbs, msgs), run(k, sc, use_kin, scans, tbs, msgs)
    for s, ((po, xo, Po), (pk, xk, Pk)) in enumerate(zip(ro, rk)):
        assert po.n_effect == pk.n_effect > 500, (s, po.n_effect, pk.n_effect)
        assert np.allclose(xo, xk, rtol=1e-8, atol=1e-9), (s, np.abs(xo - xk).max())
        assert np.allclose(Po, Pk, rtol=1e-6, atol=1e-12), (s, np.abs(Po - Pk).max())
    assert o.get_times() == k.get_times()
    scenes.compare_maps(o.map_export(), k.map_export(), rtol=1e-6, ptol=1e-7)
    o.close()
    k.close()


@pytest.mark.parametrize("use_kin", [False, True])
def test_leftovers_are_dropped_and_the_first_bucket_looks_back(use_kin):
    """The oracle alone: without the records of (i) the result is the same bit for bit; without the record of (ii) it is not."""
    sc = offconfig.scene(None, use_kin)
    scans, tbs = two_scans(sc)
    res = {}
    for name, kw in (("both", {}), ("no_leftovers", dict(leftovers=False)), ("no_lookback", dict(lookback=False))):
        o = ob.Oracle(sc.cfg(), imu_mode_only=not use_kin)
        res[name] = bits(run(o, sc, use_kin, scans, tbs, boundary_messages(sc, use_kin, scans, tbs, **kw)), o)
        o.close()
    assert res["no_leftovers"] == res["both"], "records behind a scan's last bucket were applied"
    assert res["no_lookback"][0] == res["both"][0], "scan 0 does not see scan 1's package"
    assert res["no_lookback"][1] != res["both"][1], "a record of scan 1's package stamped before scan 0's last bucket was skipped"
