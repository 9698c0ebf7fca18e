"""-m gpu: lk_traj_rpe_dev / lk_runs_rpe_dev - per-trajectory relative pose error against ground truth, on the device.

The cases are the frozen table of tests/rpecases.py, the expected records its 50-digit evaluation (tests/golden/rpe_cases.npz), the tolerances
C_T * 2^-53 * S and C_R * 2^-53 * M^2 as derived there; n_terms, n_pairs, status and - by the table's rule - worst_trans / worst_rot are compared
exactly.  The entries hand back no term list: the term SETS show through n_terms, n_pairs and the figures (tests/test_rpe_host.py compares the lists
themselves on the restatement).

Every call's inputs lie between the guard bands of tests/devguard.py, at payload offsets 8 and 16; the trajectories stand behind three leading samples
of NaN that belong to nobody (off[0] != 0), in tables of stride 104 ([t x y z r00 .. r22]) and 144 (lk_bucket_pose); the last sample of the last
trajectory ends where the table does."""
import ctypes as C

import numpy as np
import pytest

import devguard
import rpecases as rc
import scenes
import test_overlay_runs as tor
import test_replay_runs as trr
import test_runs_cloud as trc
from legkilo_amd import abi, tum

pytestmark = pytest.mark.gpu

GOLDEN = rc.golden()
RPE = abi.rpe_dtype()
REC = abi.bucket_pose_dtype()
INVALID, STATE = "error -1: ", "error -5: "
LEAD = 3
LAYOUTS = [(104, 104, 8), (144, 144, 16), (144, 104, 16), (104, 144, 8)]   # estimate stride, ground-truth stride, payload offset inside the guarded allocation


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


def table(ts, ps, rs, stride, lead=LEAD):
    """One side's samples as the bytes of a strided table behind `lead` samples of NaN -> (uint8 image, byte offsets of the first stamp, position, rotation)."""
    t = np.concatenate([np.full(lead, np.nan)] + list(ts))
    p = np.concatenate([np.full((lead, 3), np.nan)] + list(ps))
    r = np.concatenate([np.full((lead, 3, 3), np.nan)] + list(rs))
    if stride == 104:
        a = np.concatenate([t[:, None], p, r.reshape(-1, 9)], axis=1)
        return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8), 0, 8, 32
    assert stride == 144
    a = np.zeros(len(t), dtype=REC)
    a["vel"], a["first_point"] = -3.0, 99
    a["t"], a["pos"], a["rot"] = t, p, r.reshape(-1, 9)
    return np.frombuffer(a.tobytes(), dtype=np.uint8), REC.fields["t"][1], REC.fields["pos"][1], REC.fields["rot"][1]


def offsets(arrs, lead=LEAD):
    return (lead + np.r_[0, np.cumsum([len(a) for a in arrs])]).astype(np.uint64)


class Call:
    """Cases (names of the table, or case dicts) as ONE call's tables in guarded device memory."""

    def __init__(self, g, cases, layout=LAYOUTS[0], lead=LEAD):
        es, gs, off = layout
        cs = [rc.CASES[c] if isinstance(c, str) else c for c in cases]
        self.g, self.cs, self.es, self.gs = g, cs, es, gs
        e_img, *self.e = table([c["est_t"] for c in cs], [c["est_pos"] for c in cs], [c["est_rot"] for c in cs], es, lead)
        g_img, *self.q = table([c["gt_t"] for c in cs], [c["gt_pos"] for c in cs], [c["gt_rot"] for c in cs], gs, lead)
        self.eo, self.go = offsets([c["est_t"] for c in cs], lead), offsets([c["gt_t"] for c in cs], lead)
        self.ge = devguard.Guarded.input(g, e_img, offset=off, name=f"rpe est {es} {len(cs)}")
        self.gg = devguard.Guarded.input(g, g_img, offset=off, name=f"rpe gt {gs} {len(cs)}")

    def args(self):
        return [self.ge.ptr + o for o in self.e] + [self.es, self.eo] + [self.gg.ptr + o for o in self.q] + [self.gs, self.go]

    def run(self, max_dt, delta, flags):
        res = self.g.traj_rpe_dev(*self.args(), max_dt, delta, flags=flags)
        assert len(res) == len(self.cs) and not res["reserved"].any()
        self.ge.check(), self.gg.check()   # bands untouched, inputs unmodified
        return res

    def run_modes(self):
        """{(case index, q): record}: the cases share a call, not their modes - one call per distinct (max_dt, delta, flags), and a case takes its
        record from the calls of its own modes."""
        want = {}
        for i, c in enumerate(self.cs):
            for q, delta, flags in rc.modes(c):
                want.setdefault((c["max_dt"], delta, flags), []).append((i, q))
        out = {}
        for key in sorted(want):
            res = self.run(*key)
            for i, q in want[key]:
                out[(i, q)] = res[i].copy()
        return out

    def free(self):
        self.ge.free(), self.gg.free()


@pytest.fixture(scope="module")
def ratios():
    r = {"t": (0.0, None), "r": (0.0, None)}
    yield r
    print(f"\ndevice: worst ratios {r['t'][0]:.3f} at {r['t'][1]} (C_T {rc.C_T}), {r['r'][0]:.3f} at {r['r'][1]} (C_R {rc.C_R})")


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"est{l[0]}-gt{l[1]}-off{l[2]}")
def test_every_case_against_50_digits(g, layout, ratios):
    call = Call(g, rc.NAMES, layout)
    try:
        out = call.run_modes()
    finally:
        call.free()
    n = 0
    for (i, q), rec in out.items():
        name = rc.NAMES[i]
        want = rc.expected(GOLDEN, name, q)
        rt, rr = rc.check(name, rec, want)
        if rt > ratios["t"][0]:
            ratios["t"] = (rt, (name, q, layout))
        if rr > ratios["r"][0]:
            ratios["r"] = (rr, (name, q, layout))
        if name == "identical":
            assert [float(rec[f]) for f in rc.FIGURES] == [0.0] * 6, (name, q)        # estimate == ground truth: exactly 0.0
        if name in rc.RIGID:                                                            # one rigid transform: zero within the tolerance
            assert all(float(rec[f]) <= rc.tol_t(want["S"]) + float(want[f]) for f in rc.FIGURES[:3]), (name, q)
            assert all(float(rec[f]) <= rc.tol_r(want["M"]) + float(want[f]) for f in rc.FIGURES[3:]), (name, q)
            assert max(want[f] for f in rc.FIGURES[:3]) <= 4 * rc.tol_t(want["S"]) and max(want[f] for f in rc.FIGURES[3:]) <= 4 * rc.tol_r(want["M"])
        n += 1
    assert n == sum(len(rc.CASES[name]["modes"]) for name in rc.NAMES)


NEIGHBOUR_MODES = [(0.25, 0), (1.0, 0), (1, 1), (63, 1), (64, 1), (65, 1)]


def test_a_record_does_not_depend_on_its_neighbours(g):
    """One call with all cases, one with them in reversed order, and every case alone (no leading samples either): bit-equal records.  The index
    steps of 63 .. 65 read partner words another lane wrote; unordered, or with a sum that depends on the position in the call, the three differ."""
    names = rc.NAMES
    got = {}
    for order in (names, names[::-1]):
        call = Call(g, order)
        try:
            got[tuple(order)] = {m: dict(zip(order, call.run(0.01, *m))) for m in NEIGHBOUR_MODES}
        finally:
            call.free()
    scored = 0
    for name in names:
        call = Call(g, [name], lead=0)
        try:
            for m in NEIGHBOUR_MODES:
                alone = call.run(0.01, *m)[0]
                a, b = got[tuple(names)][m][name], got[tuple(names[::-1])][m][name]
                assert a.tobytes() == b.tobytes() == alone.tobytes(), (name, m)
                c = rc.CASES[name]
                want = tum.rpe(*(c[k] for k in rc.KEYS), 0.01, m[0], by_index=bool(m[1]))   # (the modes here are not all the case's own)
                assert (int(alone["n_terms"]), int(alone["n_pairs"]), int(alone["status"])) == (want["n_terms"], want["n_pairs"], want["status"]), (name, m)
                scored += int(alone["n_terms"]) > 0
        finally:
            call.free()
    assert scored > 50   # (most cases have terms under most of these modes: the comparison is not one of empty records)


def test_poisoned_pools_give_the_same_bits(g, hip_lib, scene_small, clean_env):
    call = Call(g, rc.NAMES)
    try:
        ref = [call.run(0.01, *m) for m in NEIGHBOUR_MODES]
    finally:
        call.free()
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    h = hip_lib.LegKiloHip(scene_small.cfg())
    try:
        call = Call(h, rc.NAMES)
        try:
            for m, want in zip(NEIGHBOUR_MODES, ref):
                assert call.run(0.01, *m).tobytes() == want.tobytes(), m
        finally:
            call.free()
    finally:
        h.close()


def finite_twin(c):
    """The case with every non-finite pose value replaced by an ordinary one."""
    return dict(c, **{k: np.where(np.isfinite(c[k]), c[k], 0.25) for k in ("est_pos", "est_rot", "gt_pos", "gt_rot")})


def test_non_finite_values_outside_the_terms_are_invisible(g):
    """A NaN / inf pose in a sample that is in no term - unpaired, or between the reachable steps - is never read: the record has the bits of the same
    case with ordinary values there, and they are the expected finite figures."""
    for name in ("nan_unpaired", "nan_no_term"):
        c = rc.CASES[name]
        assert not all(np.isfinite(c[k]).all() for k in ("est_pos", "est_rot"))
        a, b = Call(g, [name]), Call(g, [finite_twin(c)])
        try:
            for q, delta, flags in rc.modes(c):
                ra, rb = a.run(c["max_dt"], delta, flags)[0], b.run(c["max_dt"], delta, flags)[0]
                assert ra.tobytes() == rb.tobytes(), (name, q)
                assert int(ra["status"]) == 0 and all(np.isfinite(ra[f]) for f in rc.FIGURES) and int(ra["n_terms"]) > 0, (name, q)
                rc.check(name, ra, rc.expected(GOLDEN, name, q))
        finally:
            a.free(), b.free()


def test_non_finite_values_inside_a_term_mark_that_trajectory_only(g):
    for name in ("nan_pos_term", "nan_rot_term"):
        c = rc.CASES[name]
        around = ["noisy_origin", "n65", "rot_angles"]
        bad = Call(g, around[:2] + [name] + around[2:])
        good = Call(g, around[:2] + [finite_twin(c)] + around[2:])
        try:
            for q, delta, flags in rc.modes(c):
                rb, rg = bad.run(c["max_dt"], delta, flags), good.run(c["max_dt"], delta, flags)
                want = rc.expected(GOLDEN, name, q)
                rc.check(name, rb[2], want)
                assert int(rb[2]["status"]) == abi.LK_RPE_NONFINITE and all(np.isnan(rb[2][f]) for f in rc.FIGURES)
                assert (int(rb[2]["n_terms"]), int(rb[2]["n_pairs"]), int(rb[2]["worst_trans"]), int(rb[2]["worst_rot"])) == (want["n_terms"], want["n_pairs"], 0, 0)
                assert int(rg[2]["status"]) == 0 and np.isfinite(rg[2]["trans_rmse"])
                for i in (0, 1, 3):
                    assert rb[i].tobytes() == rg[i].tobytes() and int(rb[i]["status"]) == 0, (name, q, i)   # the neighbours' bits are unchanged
        finally:
            bad.free(), good.free()


def raw_call(g, n, et, ep, er, es, eo, gt, gp, gr, gs, go, max_dt, delta, flags, out):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = g.L.lk_traj_rpe_dev(g.h, C.c_size_t(n), ptr(et), ptr(ep), ptr(er), C.c_size_t(es), arr(eo), ptr(gt), ptr(gp), ptr(gr), C.c_size_t(gs), arr(go),
                              C.c_double(max_dt), C.c_double(delta), C.c_uint32(flags), arr(out))
    return rc_, g.L.lk_last_error(g.h).decode()


def test_refusals(g):
    names = ["n2", "n65", "midway"]
    call = Call(g, names)
    good = call.run(0.01, 1, 1)
    n = len(names)
    E, G = call.ge.ptr, call.gg.ptr
    base = dict(n=n, et=E, ep=E + 8, er=E + 32, es=104, eo=call.eo, gt=G, gp=G + 8, gr=G + 32, gs=104, go=call.go, max_dt=0.01, delta=1.0, flags=1)
    dec_e, dec_g = call.eo.copy(), call.go.copy()
    dec_e[1], dec_g[2] = dec_e[2] + 1, dec_g[1] - 1
    refusals = [
        (dict(n=0), "n_traj"), (dict(et=None), "null"), (dict(ep=None), "null"), (dict(er=None), "null argument (estimate rotations)"), (dict(gt=None), "null"),
        (dict(gp=None), "null"), (dict(gr=None), "null argument (ground truth rotations)"), (dict(eo=None), "null"), (dict(go=None), "null"), (dict(out=None), "null"),
        (dict(es=64), "estimate stride of 64"), (dict(gs=64), "ground truth stride of 64"), (dict(es=100), "estimate stride"), (dict(gs=0), "ground truth stride"),
        (dict(et=E + 4), "estimate pointers must be 8-byte aligned"), (dict(er=E + 36), "estimate rotation pointer must be 8-byte aligned"),
        (dict(gr=G + 33), "ground truth rotation pointer must be 8-byte aligned"), (dict(gp=G + 12), "ground truth pointers must be 8-byte aligned"),
        (dict(eo=dec_e), "estimate offsets decrease at trajectory 1"), (dict(go=dec_g), "ground truth offsets decrease"),
        (dict(max_dt=-1e-9), "max_dt"), (dict(max_dt=np.nan), "max_dt"),
        (dict(delta=0.0), "delta must be finite and above 0"), (dict(delta=-1.0), "delta must be finite"), (dict(delta=np.nan), "delta must be finite"),
        (dict(delta=np.inf), "delta must be finite"), (dict(delta=0.0, flags=0), "delta must be finite"), (dict(delta=-0.1, flags=0), "delta must be finite"),
        (dict(delta=np.inf, flags=0), "delta must be finite"), (dict(delta=1.5), "whole number"), (dict(delta=0.5), "whole number"),
        (dict(delta=4294967295.0), "whole number"), (dict(flags=2), "flag"), (dict(flags=3), "flag"), (dict(flags=0x80000001), "flag"),
    ]
    try:
        for change, word in refusals:
            out = np.full(n + 2, 0xFF, dtype=np.uint8).repeat(RPE.itemsize).view(RPE)
            kw = dict(base, out=out)
            kw.update(change)
            rc_, msg = raw_call(g, **kw)
            assert rc_ == -1 and word in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)), change                    # refused before anything is launched: out as it was
            assert call.run(0.01, 1, 1).tobytes() == good.tobytes(), change          # the handle is usable, a good call is right
        # a good call writes every byte of its n_traj records and nothing behind them; the largest legal index step is accepted
        out = np.full(n + 2, 0xFF, dtype=np.uint8).repeat(RPE.itemsize).view(RPE)
        rc_, msg = raw_call(g, **dict(base, out=out))
        assert rc_ == 0 and out[:n].tobytes() == good.tobytes() and devguard.sentinel_free(out[:n]) and devguard.untouched(out[n:].view(np.uint8))
        rc_, msg = raw_call(g, **dict(base, out=out, delta=4294967294.0))
        assert rc_ == 0 and not out[:n]["n_terms"].any() and out[1]["n_pairs"] == 65, msg
    finally:
        call.free()


@pytest.mark.parametrize("side", ["estimate", "ground truth"])
@pytest.mark.parametrize("what", ["decreasing", "nan"])
def test_bad_stamps_are_found_on_the_device(g, hip_lib, side, what):
    """Stamps that decrease or are not finite, in trajectories 1 AND 3 of five: LK_ERR_INVALID naming trajectory 1 and the side; the handle goes on."""
    names = ["n2", "n65", "noisy_origin", "n129", "midway"]
    key = "est_t" if side == "estimate" else "gt_t"
    cases = [rc.CASES[n] for n in names]
    good = Call(g, cases)
    try:
        want = good.run(0.01, 1, 1)
        for i in (1, 3):
            t = cases[i][key].copy()
            t[40] = {"decreasing": t[39] - 1e-6, "nan": np.nan}[what]
            cases[i] = dict(cases[i], **{key: t})
        bad = Call(g, cases)
        try:
            for delta, flags in ((1, 1), (0.25, 0)):
                with pytest.raises(hip_lib.LegKiloError, match=INVALID + f"trajectory 1: the {side} stamps"):
                    bad.run(0.01, delta, flags)
            bad.ge.check(), bad.gg.check()
        finally:
            bad.free()
        assert good.run(0.01, 1, 1).tobytes() == want.tobytes()
    finally:
        good.free()


# ---- lk_runs_rpe_dev on the six-run cases of tests/test_runs_cloud.py

@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def store():
    st = {"trr": {}, "tor": {}, "twin": {}}
    yield st
    for c in list(st["trr"].values()) + list(st["tor"].values()) + list(st["twin"].values()):
        c["g"].close()


def ground_truth(rec, rbo, seed):
    """The recorded table under a known rigid motion, with 1 mm / 1 mrad of noise, every seventh sample left out (its bucket finds no partner)."""
    rng = np.random.default_rng(seed)
    T = rc.rot([0.2, -0.1, 1.0], 0.3)
    keep = np.arange(len(rec)) % 7 != 3
    pos = rec["pos"] @ T.T + np.array([1.0, -2.0, 0.5]) + 1e-3 * rng.normal(size=(len(rec), 3))
    rots = np.array([T @ R.reshape(3, 3) @ rc.rot(rng.normal(size=3), 1e-3 * rng.normal()) for R in rec["rot"]])
    go = np.array([int(keep[:int(b)].sum()) for b in rbo], dtype=np.uint64)
    return rec["t"][keep].copy(), pos[keep].copy(), rots[keep].copy(), go


@pytest.mark.parametrize("kind,mode", [("frozen", "imu"), ("overlay", "plain")])
def test_runs_rpe_on_the_recorded_table(kind, mode, store, oracle_lib, hip_lib, scene_plain):
    tw = trc.get_case(kind, mode, store, oracle_lib, hip_lib, scene_plain)
    c, gh = tw["c"], tw["g"]
    R = len(c["runs"])
    out = trc.cloud_call(gh, kind, mode, c["runs"], c["tbs"], c["xs"], c["msgs"])   # the handle's last replay is this one
    rec = out["rec"]
    rbo = out["sbo"][np.r_[0, np.cumsum([len(run) for run in c["runs"]])]].astype(np.uint64)
    B = len(rec)
    assert int(rbo[-1]) == B and R == 6
    gt_t, gt_pos, gt_rot, go = ground_truth(rec, rbo, 5151)
    before = dict(X=out["X"], P=out["P"], times=out["times"], rec=gh.runs_bucket_poses(0, B), map=gh.map_export().copy(),
                  ov=[gh.overlay_export(r) for r in range(R)] if kind == "overlay" else None)
    gt = np.ascontiguousarray(np.concatenate([gt_t[:, None], gt_pos, gt_rot.reshape(-1, 9)], axis=1))
    ggt = devguard.Guarded.input(gh, gt, offset=8, name="runs rpe gt")
    gcp = devguard.Guarded(gh, REC.itemsize * B, offset=16, name="runs rpe table copy")
    G = (ggt.ptr, ggt.ptr + 8, ggt.ptr + 32, 104, go)
    try:
        for delta, by_index in ((0.004, False), (3, True)):
            got = gh.runs_rpe_dev(rbo, *G, 1e-4, delta, by_index=by_index)
            ggt.check()
            # the same bits as lk_traj_rpe_dev on a copy of the table
            gh.runs_bucket_poses_dev(0, B, gcp.ptr)
            twin = gh.traj_rpe_dev(*(gcp.ptr + REC.fields[f][1] for f in ("t", "pos", "rot")), 144, rbo, *G, 1e-4, delta, by_index=by_index)
            gcp.check()
            assert got.tobytes() == twin.tobytes(), (kind, delta)
            # within C of the restatement on the host copy
            for r in range(R):
                a, b, ga, gb = int(rbo[r]), int(rbo[r + 1]), int(go[r]), int(go[r + 1])
                want = tum.rpe(rec["t"][a:b], rec["pos"][a:b], rec["rot"][a:b], gt_t[ga:gb], gt_pos[ga:gb], gt_rot[ga:gb], 1e-4, delta, by_index=by_index)
                assert 0 < want["n_terms"] < want["n_pairs"] < b - a, (r, want["n_terms"], want["n_pairs"])   # every run has unpaired buckets and unscored steps
                for f in ("n_terms", "n_pairs", "status", "worst_trans", "worst_rot"):
                    assert int(got[r][f]) == want[f], (kind, delta, r, f)
                S = max(1.0, float(np.abs(rec["pos"][a:b]).max()), float(np.abs(gt_pos[ga:gb]).max()))
                M = max(1.0, float(np.abs(rec["rot"][a:b]).max()), float(np.abs(gt_rot[ga:gb]).max()))
                for f in rc.FIGURES:
                    tol = rc.tol_t(S) if f.startswith("trans") else rc.tol_r(M)
                    assert abs(float(got[r][f]) - want[f]) <= 2 * tol, (kind, delta, r, f, got[r][f], want[f])   # (either side within tol of the truth)
                assert got[r]["trans_rmse"] < 0.02 and got[r]["rot_rmse"] < 0.02   # the rigid motion does not show: millimetres and milliradians are left
        # a range past the table
        past = rbo.copy()
        past[-1] = B + 1
        with pytest.raises(hip_lib.LegKiloError, match=INVALID + "bucket range"):
            gh.runs_rpe_dev(past, *G, 1e-4, 3, by_index=True)
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
            gh.runs_rpe_dev(rbo, *G, 1e-4, 3, by_index=True)
    finally:
        ggt.free(), gcp.free()
