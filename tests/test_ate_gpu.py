"""-m gpu: lk_traj_ate_dev / lk_runs_ate_dev - per-trajectory absolute trajectory error against ground truth, on the device.

The cases are the frozen table of tests/atecases.py, the expected figures its 50-digit evaluation (tests/golden/ate_cases.npz), the tolerance
C * 2^-53 * S as derived there; n_pairs, status and - where the 50-digit values separate the worst pair from the runner-up - worst are compared exactly.
The entries hand back no pair list: the pair SETS show through n_pairs and through the unaligned figures (the positions of the stamp cases are random,
so another partner moves them by orders of magnitude more than the tolerance); tests/test_ate_host.py compares the sets themselves on the restatement.

Every call's inputs lie between the guard bands of tests/devguard.py, at payload offsets 8 and 16; the trajectories stand behind three leading samples
with NaN stamps and positions that belong to nobody (off[0] != 0), in tables of stride 32 ([t x y z]) and 144 (lk_bucket_pose)."""
import ctypes as C
import os

import numpy as np
import pytest

import ate_ref
import atecases as ac
import devguard
import scenes
import test_overlay_runs as tor
import test_replay_runs as trr
import test_runs_cloud as trc
from legkilo_amd import abi, synth

pytestmark = pytest.mark.gpu

GOLDEN = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ate_cases.npz")))
ATE = abi.ate_dtype()
REC = abi.bucket_pose_dtype()
INVALID, STATE = "error -1: ", "error -5: "
LEAD = 3
LAYOUTS = [(32, 32, 8), (144, 32, 16), (32, 144, 16)]   # estimate stride, ground-truth stride, payload offset inside the guarded allocation


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("LEGKILO_POISON_POOLS", raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def scene_small():
    return scenes.Scene(max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12)


@pytest.fixture(scope="module")
def g(hip_lib, scene_small):
    h = hip_lib.LegKiloHip(scene_small.cfg())
    yield h
    h.close()


def expected(name, flag):
    k = f"{name}/a{flag}/"
    fig, cnt = GOLDEN[k + "figures"], GOLDEN[k + "counts"]
    return dict(rmse=fig[0], mean=fig[1], max=fig[2], n_pairs=int(cnt[0]), status=int(cnt[1]), worst=int(cnt[2]), worst_margin=float(GOLDEN[k + "worst_margin"][0]),
                pairs=GOLDEN[k + "pairs"])


def table(ts, ps, stride, lead=LEAD):
    """One side's samples as the bytes of a strided table behind `lead` samples of NaN -> (uint8 image, byte offset of the first stamp, of the first position)."""
    t = np.concatenate([np.full(lead, np.nan)] + list(ts))
    p = np.concatenate([np.full((lead, 3), np.nan)] + list(ps))
    if stride == 32:
        a = np.concatenate([t[:, None], p], axis=1)
        return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8), 0, 8
    assert stride == 144
    a = np.zeros(len(t), dtype=REC)
    a["rot"], a["vel"], a["first_point"] = 7.0, -3.0, 99
    a["t"], a["pos"] = t, p
    return np.frombuffer(a.tobytes(), dtype=np.uint8), REC.fields["t"][1], REC.fields["pos"][1]


def offsets(arrs, lead=LEAD):
    return (lead + np.r_[0, np.cumsum([len(a) for a in arrs])]).astype(np.uint64)


class Call:
    """The named cases as ONE call's tables in guarded device memory."""

    def __init__(self, g, names, layout=LAYOUTS[0], lead=LEAD):
        es, gs, off = layout
        cs = [ac.CASES[n] for n in names]
        self.g, self.names, self.es, self.gs = g, names, es, gs
        e_img, self.e_t, self.e_p = table([c["est_t"] for c in cs], [c["est_pos"] for c in cs], es, lead)
        g_img, self.g_t, self.g_p = table([c["gt_t"] for c in cs], [c["gt_pos"] for c in cs], gs, lead)
        self.eo, self.go = offsets([c["est_t"] for c in cs], lead), offsets([c["gt_t"] for c in cs], lead)
        self.ge = devguard.Guarded.input(g, e_img, offset=off, name=f"ate est {es} {len(names)}")
        self.gg = devguard.Guarded.input(g, g_img, offset=off, name=f"ate gt {gs} {len(names)}")

    def run(self, flag, max_dt=None):
        """The cases share a call, not a max_dt: the call is made once per distinct max_dt and a case takes its record from its own."""
        out = np.zeros(len(self.names), dtype=ATE)
        dts = [ac.CASES[n]["max_dt"] for n in self.names] if max_dt is None else [max_dt] * len(self.names)
        for dt in sorted(set(dts)):
            res = self.g.traj_ate_dev(self.ge.ptr + self.e_t, self.ge.ptr + self.e_p, self.es, self.eo, self.gg.ptr + self.g_t, self.gg.ptr + self.g_p, self.gs,
                                      self.go, dt, flags=flag)
            assert devguard.sentinel_free(res)
            for i, d in enumerate(dts):
                if d == dt:
                    out[i] = res[i]
        self.ge.check(), self.gg.check()   # bands untouched, inputs unmodified
        return out

    def free(self):
        self.ge.free(), self.gg.free()


def check_record(name, flag, rec):
    c, want = ac.CASES[name], expected(name, flag)
    tag = (name, flag)
    assert (int(rec["n_pairs"]), int(rec["status"])) == (want["n_pairs"], want["status"]), tag
    ratio = 0.0
    for f in ("rmse", "mean", "max"):
        if np.isnan(want[f]):
            assert np.isnan(rec[f]), tag
        else:
            ratio = max(ratio, abs(float(rec[f]) - float(want[f])) / (ac.ULP * ac.scale(c)))
    assert ratio <= ac.C, (tag, ratio)
    if want["n_pairs"] and not want["status"] and want["worst_margin"] > 2 * ac.tol(c):
        assert int(rec["worst"]) == want["worst"], tag
    if not want["n_pairs"] or want["status"]:
        assert int(rec["worst"]) == 0, tag
    R, t = rec["rot"].reshape(3, 3), rec["trans"]
    if not flag or not want["n_pairs"] or want["status"]:
        assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3)), tag
    else:
        # the device's own R, t applied on the host reproduce its rmse: tests R without needing it unique
        assert abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-14, tag
        gp, pp = c["gt_pos"][want["pairs"][:, 1]], c["est_pos"][want["pairs"][:, 0]]
        d = gp - (pp @ R.T + t)
        assert abs(float(np.sqrt((d * d).sum(1).mean())) - float(rec["rmse"])) <= ac.tol(c), tag
    return ratio


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"est{l[0]}-gt{l[1]}-off{l[2]}")
@pytest.mark.parametrize("flag", ac.FLAGS)
def test_every_case_against_50_digits(g, flag, layout):
    call = Call(g, ac.NAMES, layout)
    try:
        out = call.run(flag)
    finally:
        call.free()
    worst, where = 0.0, None
    for name, rec in zip(ac.NAMES, out):
        r = check_record(name, flag, rec)
        if r > worst:
            worst, where = r, name
    print(f"flag {flag} layout {layout}: worst ratio {worst:.3f} at {where} (C {ac.C})")
    if not flag:
        z = out[ac.NAMES.index("identical")]
        assert (z["rmse"], z["mean"], z["max"]) == (0.0, 0.0, 0.0)     # estimate == ground truth: exactly 0.0


def test_a_record_does_not_depend_on_its_neighbours(g):
    """One call with all cases, one with them in another order, and every case alone (no leading samples either): bit-equal records."""
    names = ac.NAMES
    perm = [names[i] for i in np.random.default_rng(7).permutation(len(names))]
    assert perm != names
    for flag in ac.FLAGS:
        got = {}
        for order in (names, perm):
            call = Call(g, order)
            try:
                got[tuple(order)] = dict(zip(order, call.run(flag, max_dt=0.01)))
            finally:
                call.free()
        for name in names:
            call = Call(g, [name], lead=0)
            try:
                alone = call.run(flag, max_dt=0.01)[0]
            finally:
                call.free()
            a, b = got[tuple(names)][name], got[tuple(perm)][name]
            assert a.tobytes() == b.tobytes() == alone.tobytes(), (name, flag)


def test_poisoned_pools_give_the_same_bits(g, hip_lib, scene_small, clean_env):
    call = Call(g, ac.NAMES)
    try:
        ref = [call.run(flag) for flag in ac.FLAGS]
    finally:
        call.free()
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    h = hip_lib.LegKiloHip(scene_small.cfg())
    try:
        call = Call(h, ac.NAMES)
        try:
            for flag in ac.FLAGS:
                assert call.run(flag).tobytes() == ref[flag].tobytes(), flag
        finally:
            call.free()
    finally:
        h.close()


def raw_call(g, n, et, ep, es, eo, gt, gp, gs, go, max_dt, flags, out):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc = g.L.lk_traj_ate_dev(g.h, C.c_size_t(n), ptr(et), ptr(ep), C.c_size_t(es), arr(eo), ptr(gt), ptr(gp), C.c_size_t(gs), arr(go), C.c_double(max_dt),
                             C.c_uint32(flags), arr(out))
    return rc, g.L.lk_last_error(g.h).decode()


def test_refusals(g):
    names = ["n3", "n65", "midway"]
    call = Call(g, names)
    good = [call.run(flag, max_dt=0.01) for flag in ac.FLAGS]
    n = len(names)
    base = dict(n=n, et=call.ge.ptr, ep=call.ge.ptr + 8, es=32, eo=call.eo, gt=call.gg.ptr, gp=call.gg.ptr + 8, gs=32, go=call.go, max_dt=0.01, flags=1)
    dec_e, dec_g = call.eo.copy(), call.go.copy()
    dec_e[1], dec_g[2] = dec_e[2] + 1, dec_g[1] - 1
    refusals = [
        (dict(n=0), "n_traj"), (dict(et=None), "null"), (dict(ep=None), "null"), (dict(gt=None), "null"), (dict(gp=None), "null"), (dict(eo=None), "null"),
        (dict(go=None), "null"), (dict(out=None), "null"), (dict(es=20), "estimate stride"), (dict(es=16), "estimate stride"), (dict(gs=0), "ground truth stride"),
        (dict(gs=36), "ground truth stride"), (dict(et=call.ge.ptr + 4), "aligned"), (dict(eo=dec_e), "estimate offsets decrease at trajectory 1"),
        (dict(go=dec_g), "ground truth offsets decrease"), (dict(max_dt=-1e-9), "max_dt"), (dict(max_dt=np.nan), "max_dt"), (dict(max_dt=np.inf), "max_dt"),
        (dict(flags=2), "flag"), (dict(flags=0x80000001), "flag"),
    ]
    try:
        for change, word in refusals:
            out = np.full(n + 2, 0xFF, dtype=np.uint8).repeat(ATE.itemsize).view(ATE)
            kw = dict(base, out=out)
            kw.update(change)
            rc, msg = raw_call(g, **kw)
            assert rc == -1 and word in msg, (change, rc, msg)
            assert devguard.untouched(out.view(np.uint8)), change                 # refused before anything is launched: out as it was
            assert call.run(1, max_dt=0.01).tobytes() == good[1].tobytes(), change   # the handle is usable, a good call is right
        # out past n_traj records stays untouched by a good call
        out = np.full(n + 2, 0xFF, dtype=np.uint8).repeat(ATE.itemsize).view(ATE)
        rc, msg = raw_call(g, **dict(base, out=out))
        assert rc == 0 and out[:n].tobytes() == good[1].tobytes() and devguard.untouched(out[n:].view(np.uint8))
    finally:
        call.free()


@pytest.mark.parametrize("side", ["estimate", "ground truth"])
@pytest.mark.parametrize("what", ["decreasing", "nan", "inf"])
def test_bad_stamps_are_found_on_the_device(g, hip_lib, side, what):
    """Stamps that decrease or are not finite, in trajectories 1 AND 3 of five: LK_ERR_INVALID naming trajectory 1 and the side; the handle goes on."""
    names = ["n3", "n65", "arc_origin", "n129", "midway"]
    key = "est_t" if side == "estimate" else "gt_t"
    saved = {n: ac.CASES[n][key] for n in ("n65", "n129")}
    good = Call(g, names)
    try:
        want = good.run(1, max_dt=0.01)
        for n in saved:
            t = saved[n].copy()
            t[40] = {"decreasing": t[39] - 1e-6, "nan": np.nan, "inf": np.inf}[what]
            if what == "inf":
                t[41:] = np.inf   # (still not decreasing: the stamp is refused for being infinite)
            ac.CASES[n] = dict(ac.CASES[n], **{key: t})
        bad = Call(g, names)
        try:
            with pytest.raises(hip_lib.LegKiloError, match=INVALID + f"trajectory 1: the {side} stamps"):
                bad.run(1, max_dt=0.01)
            bad.ge.check(), bad.gg.check()
        finally:
            bad.free()
        assert good.run(1, max_dt=0.01).tobytes() == want.tobytes()
    finally:
        for n, t in saved.items():
            ac.CASES[n] = dict(ac.CASES[n], **{key: t})
        good.free()


# ---- lk_runs_ate_dev on the six-run cases of tests/test_runs_cloud.py

@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def store():
    st = {"trr": {}, "tor": {}, "twin": {}}
    yield st
    for c in list(st["trr"].values()) + list(st["tor"].values()) + list(st["twin"].values()):
        c["g"].close()


def run_ranges(c, sbo):
    ro = np.r_[0, np.cumsum([len(run) for run in c["runs"]])]
    return sbo[ro].astype(np.uint64)


def ground_truth(rec, rbo, seed):
    """The recorded table under a known rigid motion with 1 mm of noise, every seventh sample left out (its bucket finds no partner within max_dt)."""
    rng = np.random.default_rng(seed)
    R = ac.rot([0.2, -0.1, 1.0], 0.3)
    keep = np.arange(len(rec)) % 7 != 3
    pos = rec["pos"] @ R.T + np.array([1.0, -2.0, 0.5]) + 1e-3 * rng.normal(size=(len(rec), 3))
    go = np.array([int(keep[:int(b)].sum()) for b in rbo], dtype=np.uint64)
    return rec["t"][keep].copy(), pos[keep].copy(), go


@pytest.mark.parametrize("kind,mode", [("frozen", "imu"), ("overlay", "plain")])
def test_runs_ate_on_the_recorded_table(kind, mode, store, oracle_lib, hip_lib, scene_plain):
    tw = trc.get_case(kind, mode, store, oracle_lib, hip_lib, scene_plain)
    c, gh = tw["c"], tw["g"]
    R = len(c["runs"])
    out = trc.cloud_call(gh, kind, mode, c["runs"], c["tbs"], c["xs"], c["msgs"])   # the handle's last replay is this one
    rec, rbo = out["rec"], run_ranges(c, out["sbo"])
    B = len(rec)
    assert int(rbo[-1]) == B and R == 6
    gt_t, gt_pos, go = ground_truth(rec, rbo, 5150)
    before = dict(X=out["X"], P=out["P"], times=out["times"], rec=gh.runs_bucket_poses(0, B), map=gh.map_export().copy(),
                  ov=[gh.overlay_export(r) for r in range(R)] if kind == "overlay" else None)
    gt = np.ascontiguousarray(np.concatenate([gt_t[:, None], gt_pos], axis=1))
    ggt = devguard.Guarded.input(gh, gt, offset=8, name="runs ate gt")
    gcp = devguard.Guarded(gh, REC.itemsize * B, offset=16, name="runs ate table copy")
    try:
        for flag in ac.FLAGS:
            got = gh.runs_ate_dev(rbo, ggt.ptr, ggt.ptr + 8, 32, go, 1e-4, flags=flag)
            ggt.check()
            # the same bits as lk_traj_ate_dev on a copy of the table
            gh.runs_bucket_poses_dev(0, B, gcp.ptr)
            twin = gh.traj_ate_dev(gcp.ptr + REC.fields["t"][1], gcp.ptr + REC.fields["pos"][1], 144, rbo, ggt.ptr, ggt.ptr + 8, 32, go, 1e-4, flags=flag)
            gcp.check()
            assert got.tobytes() == twin.tobytes(), (kind, flag)
            assert got.tobytes() == gh.runs_ate(rbo, gt_t, gt_pos, go, 1e-4, align=bool(flag)).tobytes()
            # within C of the restatement on the host copy
            for r in range(R):
                case = ac.case(rec["t"][int(rbo[r]):int(rbo[r + 1])], rec["pos"][int(rbo[r]):int(rbo[r + 1])], gt_t[int(go[r]):int(go[r + 1])],
                               gt_pos[int(go[r]):int(go[r + 1])], 1e-4)
                want = ate_ref.ate(case, flag)
                assert 0 < want["n_pairs"] < len(case["est_t"]), (r, want["n_pairs"])   # every run has paired and unpaired buckets
                assert (int(got[r]["n_pairs"]), int(got[r]["status"])) == (want["n_pairs"], 0), (kind, flag, r)
                for f in ("rmse", "mean", "max"):
                    assert abs(float(got[r][f]) - want[f]) <= ac.tol(case), (kind, flag, r, f, got[r][f], want[f])
                if flag:
                    assert got[r]["rmse"] < 5e-3 < ate_ref.ate(case, 0)["rmse"]   # the rigid motion is removed: the millimetre of noise is left
        # a range past the table
        past = rbo.copy()
        past[-1] = B + 1
        with pytest.raises(hip_lib.LegKiloError, match=INVALID + "bucket range"):
            gh.runs_ate_dev(past, ggt.ptr, ggt.ptr + 8, 32, go, 1e-4)
        # nothing else moved
        X, P = gh.batch_get_states(0, R)
        assert np.array_equal(X, before["X"]) and np.array_equal(P, before["P"]) and trr.times_of(gh, R) == before["times"]
        assert trc.same_records(gh.runs_bucket_poses(0, B), before["rec"]) and np.array_equal(gh.map_export(), before["map"])
        if kind == "overlay":
            for r in range(R):
                assert scenes.maps_identical(gh.overlay_export(r), before["ov"][r]), r
        # a plain replay records nothing
        if kind == "frozen":
            gh.batch_replay_runs(c["runs"], c["tbs"], c["xs"], [trr.P0] * R, **tor.msg_kw(mode, c["msgs"]))
        else:
            gh.batch_replay_overlay_runs(c["runs"], c["tbs"], c["xs"], [trr.P0] * R, **tor.msg_kw(mode, c["msgs"]))
        with pytest.raises(hip_lib.LegKiloError, match=STATE + ".*recorded no bucket poses"):
            gh.runs_ate_dev(rbo, ggt.ptr, ggt.ptr + 8, 32, go, 1e-4)
    finally:
        ggt.free(), gcp.free()


def test_choose_a_slot_and_commit_it(store, oracle_lib, hip_lib, scene_plain):
    """The windowed-mapping recipe, small: one three-scan window replayed with insert on three slots from three priors - the true state, and the true
    state moved by 50 cm and by 25 cm; lk_runs_ate_dev against the true trajectory ranks the undisturbed prior best; that slot's overlay commits."""
    c = trc.get_case("overlay", "plain", store, oracle_lib, hip_lib, scene_plain)["c"]
    sc, run, tbs = c["sc"], c["runs"][0], c["tbs"][0]
    assert len(run) == 3
    x0 = synth.initial_state(sc.traj, tbs[0], sc.P)
    xs = [x0.copy() for _ in range(3)]
    xs[0][9:12] += np.array([0.4, -0.3, 0.0])
    xs[2][9:12] += np.array([-0.15, 0.2, 0.0])
    gh = trc.new_handle(hip_lib, c, 3)
    try:
        poses, ex = gh.batch_replay_overlay_runs([run] * 3, [tbs] * 3, xs, [trr.P0] * 3, bucket_poses=True)
        rec, sbo = ex["bucket_poses"], ex["scan_bucket_off"]
        rbo = sbo[[0, 3, 6, 9]].astype(np.uint64)
        n = int(rbo[1])
        assert np.array_equal(np.diff(rbo.astype(np.int64)), [n, n, n])
        gt_t = rec["t"][:n].copy()
        got = gh.runs_ate(rbo, np.tile(gt_t, 3), np.tile(sc.traj.pos(gt_t), (3, 1)), np.array([0, n, 2 * n, 3 * n]), 1e-6)
        print("rmse per prior (moved 50 cm, true, moved 25 cm):", got["rmse"])
        assert np.all(got["n_pairs"] == n) and np.all(got["status"] == 0)
        assert int(np.argmin(got["rmse"])) == 1
        gh.overlay_commit(1)
        assert gh.map_stats() is not None
    finally:
        gh.close()
