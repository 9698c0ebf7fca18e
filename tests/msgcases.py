"""Crafted IMU / kinematic + IMU message streams for the message-update tests (tests/test_message_edges.py on the device,
test_kilo_process_matches_the_reference_on_message_edges in tests/test_reference_pin.py for the oracle that checks them).

synth.kin_stream / synth.imu_stream never produce what goes wrong in a message kernel or in the rule that hands a message to a bucket:

  masks      the trot has the contact masks 1001, 0110 and 1111 only.  kin_all_masks writes all 16 into every scan's stream (so every row count
             M = 6 + 3 c, c = 0..4, and every case where a contact's row block is not at its leg's index), a set bit as 1, 2, -1 or 256
             (`contact` is an int tested != 0, KILO.cc:290), and leaves the swing legs' foot data in place (it must be ignored).
  ties       KILO::process applies a message iff stamp < cur_point_time (KILO.cc:379-390).  put_on_bucket_times moves every second message
             exactly onto a bucket time and makes one pair of equal stamps (dt = 0 between two messages).
  epoch      shift_times adds 1.7e9 s - the size of a recorded run's stamps, where a double resolves 2.4e-7 s - to the scan's begin time, the
             stamps and the filter's times, after everything else was generated at t ~ 3 s: the same scans and noise, but consecutive buckets of
             a scan collapse onto one absolute time (dt = 0 predicts) and stamps meet bucket times by rounding alone.
  dense      dense_with_messages: four buckets of 600 points (above the single-launch limit of 512) with a message exactly on the next
             bucket's time: the host loop of the per-bucket launches lets that bucket's predict ride unless a message lies STRICTLY before its time
             (`rides` replays the loop's decisions on an input).

The input conditions (every mask present, enough ties, enough equal bucket times, and that ties and masks change the oracle's answer by far
more than a test's tolerance) are checked by `assert_conditions` on the oracle alone, before a test looks at a device result.
"""
import functools

import numpy as np

import scenes
from legkilo_amd import config, synth

EPOCH = 1.7e9
PARAMS = dict(config.DITER, voxel_grid_resolution=0.3)
CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
SET_BIT = (1, 2, -1, 256)
# Start of the live case (the ids "t1" / "epoch" name the size of the stamps: seconds, or seconds + 1.7e9).  Chosen on the oracle alone: two IMU updates
# and a bucket's update at one time nearly commute, so at most start times a tied IMU stamp moved one ulp down changes the first scan's state by 1e-6 ..
# 9e-5 only (t0 = 1, 2, 5, 21, 31); from t0 = 3 it changes a match decision and the state by 2.9e-3, the kinematic streams' ties by 3.4e-2.
T0 = 3.0
N_LIVE = 4          # scans of the live case (first frame + N_LIVE scans with insert)
S_REPLAY = 4        # scans of the replay case (priors on a mature map)
REPLAY_GAP = 0.12   # start-time distance of the replay case's scans: consecutive enough to form runs


def scene():
    return scenes.Scene(params=PARAMS, **CAPS)


def stamp_name(msgs):
    return "time_stamp" if "time_stamp" in msgs.dtype.names else "stamp"


def bucket_times(ds, tb):
    """Absolute time of every bucket as KILO.cc:376 forms it: begin_time + (double)curvature."""
    return tb + synth.buckets_of(ds)[1]


def masks_of(kins):
    return ((kins["contact"] != 0) * (1 << np.arange(4))).sum(1)


def put_on_bucket_times(stamps, T):
    """Every second stamp (1, 3, ...) onto the first bucket time at or behind it, where that keeps the stream sorted; then one pair of equal
    stamps: stamps[20] = stamps[19] (a stream of 20 messages: stamps[10] = stamps[9]; an odd index, so the pair sits on a bucket time)."""
    s = np.array(stamps, dtype=np.float64)
    for j in range(1, len(s), 2):
        i = int(np.searchsorted(T, s[j], side="left"))
        if i < len(T) and (j + 1 == len(s) or T[i] < s[j + 1]):
            s[j] = T[i]
    p = 20 if len(s) > 20 else len(s) // 2
    s[p] = s[p - 1]
    assert np.all(np.diff(s) >= 0)
    return s


def kin_all_masks(sc, tb, k, ds):
    """Scan k's 50 kinematic + IMU messages: mask (7 i + 3 k) % 16 on message i (FR = bit 0), a set bit written as SET_BIT[(i + leg) % 4], swing
    legs' foot data as generated, every second stamp on a bucket time of `ds`."""
    kins = synth.kin_stream(sc.traj, tb, tb + 0.1, sc.P, seed=3003 + k)
    for i in range(len(kins)):
        m = (7 * i + 3 * k) % 16
        kins["contact"][i] = [SET_BIT[(i + leg) % 4] if (m >> leg) & 1 else 0 for leg in range(4)]
    kins["time_stamp"] = put_on_bucket_times(kins["time_stamp"], bucket_times(ds, tb))
    return kins


def imu_on_buckets(sc, tb, k, ds):
    imus = synth.imu_stream(sc.traj, tb, tb + 0.1, seed=3003 + k)
    imus["stamp"] = put_on_bucket_times(imus["stamp"], bucket_times(ds, tb))
    return imus


def messages(kind, sc, tb, k, ds):
    return (kin_all_masks if kind == "kin" else imu_on_buckets)(sc, tb, k, ds)


def shift_times(D, tb, msgs):
    """(tb + D, the messages stamped + D): the oracle and the device receive the same rounded doubles."""
    out = msgs.copy()
    out[stamp_name(out)] = out[stamp_name(out)] + D
    return tb + D, out


def rides(T, stamps, sizes, small_max=512):
    """The decisions of the per-bucket launches' host loop (run_scan_launches, KILO.cc:379-390 around it), replayed on an input: the queue is popped
    while stamp < T[k]; bucket k + 1's predict rides in bucket k's launch iff the queue's head is not < T[k + 1] and both buckets hold more than
    small_max points.  Returns [(rides, head stamp or None)] for k = 0 .. len(T) - 2."""
    q, out = 0, []
    for k in range(len(T) - 1):
        while q < len(stamps) and stamps[q] < T[k]:
            q += 1
        between = q < len(stamps) and stamps[q] < T[k + 1]
        out.append((bool(not between and sizes[k] > small_max and sizes[k + 1] > small_max), float(stamps[q]) if q < len(stamps) else None))
    return out


def dense_with_messages(sc, tb, kind):
    """One scan of four buckets of 600 points and three messages: none between T0 and T1 - bucket 1's predict rides in bucket 0's launch -, none
    inside (T1, T2) and one stamped exactly T2 - the queue's head is not "before" bucket 2, so bucket 2's predict rides in bucket 1's launch too, and
    the message is applied in front of bucket 3, at the time the filter already stands at -, two strictly inside (T2, T3): nothing rides into bucket
    2's launch.  rides() on the result: True (head T2), True (head == T2, the next bucket's own time), False."""
    ds = synth.dense_scan(sc.world, sc.traj, tb, sc.P, n=2400, n_buckets=4)
    T = bucket_times(ds, tb)
    assert len(T) == 4 and np.all(np.diff(T) > 0)
    msgs = (synth.kin_stream(sc.traj, tb, tb + 0.1, sc.P, seed=3103) if kind == "kin" else synth.imu_stream(sc.traj, tb, tb + 0.1, seed=3103))[:3].copy()
    if kind == "kin":
        msgs["contact"] = [[256, 1, 0, 2], [0, 2, 0, -1], [0, 0, 1, 0]]   # 1011 (M = 15), 1010, 0100
    msgs[stamp_name(msgs)] = [T[2], T[2] + (T[3] - T[2]) / 3, T[2] + 2 * (T[3] - T[2]) / 3]
    # a jolt on the tied message: an IMU update and a bucket's update at one time nearly commute, and the larger innovation is what makes their order
    # visible in the state (IMU mode: 3e-5 without it)
    msgs["acc"][0] += [1.5, -1.0, 2.0]
    msgs["gyr"][0] += [0.3, -0.2, 0.25]
    return ds, msgs


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def kin_rows(x36, rec, P, acc_norm=9.81):
    """The observation of one kinematic + IMU record at state x36 as KILO.cc:267-309 builds it: (H [M, 30], z [M], R [M]), M = 6 + 3 c; the
    c feet in contact take the row blocks 0 .. c - 1 in leg order."""
    R = x36[:9].reshape(3, 3)
    vel, ba, bw, imu_a, imu_w = x36[12:15], x36[15:18], x36[18:21], x36[24:27], x36[27:30]
    legs = [leg for leg in range(4) if rec["contact"][leg] != 0]
    M = 6 + 3 * len(legs)
    H, z, Rn = np.zeros((M, 30)), np.zeros(M), np.zeros(M)
    for i in range(6):
        H[i, 9 + i] = H[i, 18 + i] = 1.0
    z[:3] = (P["gravity"] / acc_norm) * rec["acc"] - imu_a - ba
    z[3:6] = rec["gyr"] - imu_w - bw
    Rn[:6] = [P["imu_acc_meas_noise"], P["imu_acc_meas_noise"], P["imu_acc_z_meas_noise"]] + [P["imu_gyr_meas_noise"]] * 3
    for idx, leg in enumerate(legs):
        r0 = 6 + 3 * idx
        fp, fv = rec["foot_pos"][leg], rec["foot_vel"][leg]
        wpv = skew(imu_w) @ fp + fv
        H[r0:r0 + 3, 0:3] = -R @ skew(wpv)
        H[r0:r0 + 3, 6:9] = np.eye(3)
        H[r0:r0 + 3, 21:24] = -R @ skew(fp)
        z[r0:r0 + 3] = -vel - R @ wpv
        Rn[r0:r0 + 3] = P["kin_meas_noise"]
    return H, z, Rn


def one_message_per_mask(sc, t):
    """16 kinematic + IMU records at t, one per contact mask, set bits written as in kin_all_masks, every leg's foot data present."""
    kins = synth.kin_stream(sc.traj, t, t + 0.032, sc.P, seed=3203)
    assert len(kins) == 16
    for i in range(16):
        kins["contact"][i] = [SET_BIT[(i + leg) % 4] if (i >> leg) & 1 else 0 for leg in range(4)]
    return kins


# ----------------------------------------------------------------------------- what the conditions compare the oracle with
def ties_moved_down(msgs, T):
    """Every stamp that equals a bucket time one ulp earlier: what `<=` in place of `<` would make of the stream."""
    out = msgs.copy()
    s = out[stamp_name(out)]
    tied = np.isin(s, T)
    s[tied] = np.nextafter(s[tied], -np.inf)
    return out


def contact_equals_one(kins):
    out = kins.copy()
    out["contact"] = (kins["contact"] == 1).astype(np.int32)
    return out


def three_contacts_lose_a_foot(kins):
    out = kins.copy()
    for i in np.flatnonzero((kins["contact"] != 0).sum(1) == 3):
        out["contact"][i, np.flatnonzero(kins["contact"][i])[-1]] = 0
    return out


def leg1_reads_leg0(kins):
    """Messages whose mask holds leg 1 but neither leg 0 nor leg 2 (leg 1's rows are contact block 0): leg 1 gets leg 0's foot data - what a
    kernel would compute that read the foot data at the row block's index."""
    out = kins.copy()
    m = masks_of(kins)
    sel = ((m & 0b0111) == 0b0010)
    out["foot_pos"][sel, 1] = kins["foot_pos"][sel, 0]
    out["foot_vel"][sel, 1] = kins["foot_vel"][sel, 0]
    return out


KIN_VARIANTS = dict(contact_equals_one=contact_equals_one, three_contacts_lose_a_foot=three_contacts_lose_a_foot, leg1_reads_leg0=leg1_reads_leg0)


# ----------------------------------------------------------------------------- the cases (built once, shared, never changed)
class Case:
    """scans: list of dict(ds, tb, msgs, T) with absolute times; x0 / xs: priors; blob: the map the replay starts from; decides: name ->
    max |dx| after the first scan between the oracle on the case's messages and on a variant of them."""


def _kw(kind, msgs):
    return {"kins" if kind == "kin" else "imus": msgs}


def _scan(kind, sc, tb, k, epoch, edge=None):
    """edge: the scan's second bucket ("head") or its last but one ("tail") moved to within 1e-7 s of its neighbour at the scan's end - two
    buckets at t ~ 3 s, one absolute time at 1.7e9 s.  (The generator's first and last bucket lie 3e-4 s from their neighbours.)"""
    ds = scenes.vlp_scan_input(sc, tb, k)
    if edge is not None:
        off, dt = synth.buckets_of(ds)
        b = 1 if edge == "head" else len(dt) - 2
        near = np.float32(1e-7) if edge == "head" else np.nextafter(ds["curvature"][-1], np.float32(0))
        assert ds["curvature"][off[b] - 1] < near < ds["curvature"][off[b + 1]]
        ds["curvature"][off[b]:off[b + 1]] = near
    msgs = messages(kind, sc, tb, k, ds)
    if epoch:
        tb, msgs = shift_times(EPOCH, tb, msgs)
    return dict(ds=ds, tb=tb, msgs=msgs, T=bucket_times(ds, tb), k=k)


def _decides(kind, scan0, first_scan_state):
    base = first_scan_state(scan0["msgs"])
    variants = dict(ties_moved_down=ties_moved_down(scan0["msgs"], scan0["T"]))
    if kind == "kin":
        variants.update({n: f(scan0["msgs"]) for n, f in KIN_VARIANTS.items()})
    return {n: float(np.abs(first_scan_state(m) - base).max()) for n, m in variants.items()}


@functools.lru_cache(maxsize=None)
def live_case(kind, epoch):
    """First frame at T0 and N_LIVE config-1 scans with insert, crafted messages; the oracle's run of it (per scan: counts, state, times; final
    P and map)."""
    import oracle_binding as ob

    c = Case()
    c.kind, c.epoch, c.sc = kind, epoch, scene()
    c.t0 = T0 + (EPOCH if epoch else 0.0)
    c.scans = [_scan(kind, c.sc, T0 + 0.1 * k, k, epoch) for k in range(N_LIVE)]

    def started():
        o = ob.Oracle(c.sc.cfg(), imu_mode_only=kind != "kin")
        start(o, c)
        return o

    o = started()
    c.oracle = []
    for s in c.scans:
        po, _ = o.process_scan(s["ds"], s["tb"], **_kw(kind, s["msgs"]))
        c.oracle.append(((po.n_buckets, po.n_updates, int(po.n_effect)), o.get_state()[0].copy(), o.get_times()))
    c.oracle_P, c.oracle_map = o.get_state()[1].copy(), o.map_export()
    o.close()

    def first_scan_state(msgs):
        o = started()
        o.process_scan(c.scans[0]["ds"], c.scans[0]["tb"], **_kw(kind, msgs))
        x = o.get_state()[0].copy()
        o.close()
        return x

    c.decides = _decides(kind, c.scans[0], first_scan_state)
    return c


def start(obj, c):
    """Filter at the trajectory's state at T0, times at the case's t0, first-frame map."""
    x0 = scenes.init_filter(obj, c.sc, T0)
    obj.set_times(c.t0, c.t0)
    scenes.first_frame(obj, c.sc, T0, x0)


@functools.lru_cache(maxsize=None)
def replay_case(kind, epoch):
    """S_REPLAY config-1 scans with perturbed priors and crafted messages on the map the oracle holds after the live case at t ~ 3 s (the idiom of
    test_batch_replay_ragged_leg_fusion).  Scan s begins REPLAY_GAP behind scan s - 1: scans 0, 1 and 2, 3 also form two runs."""
    import oracle_binding as ob

    c = Case()
    c.kind, c.epoch, c.sc = kind, epoch, scene()
    rng = np.random.default_rng(4242)
    c.scans, c.xs = [], []
    for s in range(S_REPLAY):
        tb = T0 + 0.5 + REPLAY_GAP * s
        c.scans.append(_scan(kind, c.sc, tb, 70 + s, epoch, edge="head" if s % 2 else "tail"))   # runs of two scans: equal times on both sides of the boundary
        c.xs.append(synth.initial_state(c.sc.traj, tb, c.sc.P, rng, 0.02, 0.5))
    c.P0 = 1e-4 * np.eye(30)
    o = ob.Oracle(c.sc.cfg(), imu_mode_only=kind != "kin")
    o.map_import(live_case(kind, False).oracle_map)
    c.blob = o.map_export()   # the form a blob round trip leaves the map in (see test_batch_replay_overlay): what checker and device both start from
    o.init_process_cov_q()
    o.set_acc_norm(9.81)
    o.set_map_insert(False)

    def frozen(s, msgs):
        o.set_state(c.xs[s], c.P0)
        o.set_times(c.scans[s]["tb"], c.scans[s]["tb"])
        po, _ = o.process_scan(c.scans[s]["ds"], c.scans[s]["tb"], **_kw(kind, msgs))
        x, P = o.get_state()
        return (po.n_buckets, po.n_updates, int(po.n_effect)), x.copy(), P.copy()

    c.oracle_frozen = [frozen(s, c.scans[s]["msgs"]) for s in range(S_REPLAY)]
    c.decides = _decides(kind, c.scans[0], lambda msgs: frozen(0, msgs)[1])
    o.close()
    return c


@functools.lru_cache(maxsize=None)
def overlay_oracle(kind, epoch):
    """The replay case scan by scan WITH the insert, each scan on a private copy of the case's map: per slot (counts, x, P, canon map after)."""
    import oracle_binding as ob

    c = replay_case(kind, epoch)
    o = ob.Oracle(c.sc.cfg(), imu_mode_only=kind != "kin")
    o.init_process_cov_q()
    o.set_acc_norm(9.81)
    out = []
    for s, scan in enumerate(c.scans):
        o.map_import(c.blob)
        o.set_map_insert(True)
        o.set_state(c.xs[s], c.P0)
        o.set_times(scan["tb"], scan["tb"])
        po, _ = o.process_scan(scan["ds"], scan["tb"], **_kw(kind, scan["msgs"]))
        x, P = o.get_state()
        out.append(((po.n_buckets, po.n_updates, int(po.n_effect)), x.copy(), P.copy(), scenes.canon_map(o.map_export())))
    o.close()
    return out


def assert_conditions(c, xtol):
    """The input conditions of a case, for a test whose state tolerance is xtol.  Nothing here looks at a device result."""
    for s in c.scans:
        st = s["msgs"][stamp_name(s["msgs"])]
        assert np.all(np.diff(st) >= 0) and (np.diff(st) == 0).sum() >= 1, "time-sorted, with one pair of equal stamps"
        if c.kind == "kin":
            assert set(masks_of(s["msgs"])) == set(range(16)), s["k"]
        if c.epoch:
            pairs = int((np.diff(s["T"]) == 0).sum())
            assert pairs >= 20, (s["k"], pairs)
            assert np.isin(st, s["T"]).sum() >= 1, s["k"]   # (tb + D) + c and (tb + c) + D may round apart: some stamp still meets a bucket time
        else:
            on = int(np.isin(st, s["T"]).sum())
            assert on >= (20 if c.kind == "kin" else 6), (s["k"], on)
    n_effect = [r[0][2] for r in (c.oracle if hasattr(c, "oracle") else c.oracle_frozen)]
    assert min(n_effect) > 500, n_effect
    for name, d in c.decides.items():
        assert d >= 1e3 * xtol, (c.kind, c.epoch, name, d, xtol)
