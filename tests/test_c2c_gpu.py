"""-m gpu: lk_clouds_c2c_dev / lk_clouds_c2c - cloud-to-cloud nearest-neighbour distance of many pairs of clouds, on the device.

The cases are the frozen table of tests/c2ccases.py, the expected values its 50-digit evaluation (tests/golden/c2c_cases.npz): j(i), matched flags,
n_matched, n_within, worst and status are compared exactly, rmse / mean / max within C * 2^-53 * max_dist as derived there; the nn arrays are compared
bit for bit with the brute force of legkilo_amd.cloudmetrics.

Every call's clouds lie between the guard bands of tests/devguard.py at payload offset 16, behind three leading records of NaN that belong to nobody
(off[0] != 0) and in front of one more cloud of NaN that no pair names; every record's w is NaN (never read).  The nn arrays are guarded outputs of
exactly nn_off[n_pairs] entries, so a write behind them lands in a band."""
import ctypes as C

import numpy as np
import pytest

import c2ccases as cc
import devguard
import scenes
import test_map_clouds as tmc
import test_overlay_runs as tor
import test_replay_runs as trr
from legkilo_amd import abi, cloudmetrics

pytestmark = pytest.mark.gpu

GOLDEN = cc.golden()
REC = abi.c2c_dtype()
LEAD = 3
FIGURES = ("rmse", "mean", "max")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("LEGKILO_POISON_POOLS", raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def g(hip_lib):
    h = tmc.new_handle(hip_lib)
    yield h
    h.close()


@pytest.fixture(scope="module")
def brute():
    """cloudmetrics.c2c of every case, once, shared and left unchanged."""
    return {n: cloudmetrics.c2c(c["query"], c["ref"], c["max_dist"], c["thr"]) for n, c in cc.CASES.items()}


def side(clouds, lead=LEAD):
    """Clouds [n_i, 3] as one buffer of x y z w records: `lead` records of NaN, the clouds, one more cloud of two NaN records that no pair names.
    -> (float32 [N, 4], offsets uint64 [len(clouds) + 2])."""
    parts = [np.full((lead, 3), np.nan, dtype=np.float32)] + [np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds] + [np.full((2, 3), np.nan, dtype=np.float32)]
    xyz = np.concatenate(parts)
    rec = np.full((len(xyz), 4), np.nan, dtype=np.float32)
    rec[:, :3] = xyz
    off = (lead + np.r_[0, np.cumsum([len(p) for p in parts[1:]])]).astype(np.uint64)
    return rec, off


class Call:
    """Cases (names of the table) as ONE call in guarded device memory: pair i = (query cloud i, reference cloud i), then `extra` pairs of cloud
    indices - clouds shared by several pairs; the last cloud of either side is in no pair."""

    def __init__(self, g, names, extra=(), with_nn=True):
        self.g, self.names = g, list(names)
        cs = [cc.CASES[n] for n in names]
        self.max_dist, self.thr = cs[0]["max_dist"], cs[0]["thr"]
        assert all(c["max_dist"] == self.max_dist and np.array_equal(c["thr"], self.thr) for c in cs)
        self.q, self.qo = side([c["query"] for c in cs])
        self.r, self.ro = side([c["ref"] for c in cs])
        self.pairs = np.array([(i, i) for i in range(len(cs))] + list(extra), dtype=np.uint32).reshape(-1, 2)
        self.total = int(sum(int(self.qo[a + 1] - self.qo[a]) for a, _ in self.pairs))
        tag = f"c2c {names[0]} {len(names)} {len(extra)}"
        self.gq = devguard.Guarded.input(g, self.q, offset=16, name=tag + " query")
        self.gr = devguard.Guarded.input(g, self.r, offset=16, name=tag + " ref")
        self.gi = devguard.Guarded(g, 4 * self.total, offset=4, name=tag + " nn_idx") if with_nn else None
        self.gd = devguard.Guarded(g, 8 * self.total, offset=8, name=tag + " nn_d2") if with_nn else None

    def run(self):
        """-> (records, nn_off, nn_idx, nn_d2); bands untouched, inputs unmodified."""
        res, nn_off = self.g.clouds_c2c_dev(self.gq.ptr, self.qo, self.gr.ptr, self.ro, self.pairs, self.max_dist, self.thr,
                                            self.gi.ptr if self.gi else 0, self.gd.ptr if self.gd else 0)
        self.gq.check(), self.gr.check()
        assert len(res) == len(self.pairs) and int(nn_off[0]) == 0 and int(nn_off[-1]) == self.total
        assert np.array_equal(np.diff(nn_off.astype(np.int64)), [int(self.qo[a + 1] - self.qo[a]) for a, _ in self.pairs])
        if not self.gi:
            return res, nn_off, None, None
        idx, d2 = self.gi.read(np.uint32), self.gd.read(np.float64)     # (check(): nothing behind nn_off[n_pairs] entries was written)
        assert len(idx) == len(d2) == self.total
        if self.total:
            assert devguard.sentinel_free(d2) and not np.isnan(d2).any()
        return res, nn_off, idx, d2

    def free(self):
        for b in (self.gq, self.gr, self.gi, self.gd):
            if b:
                b.free()


def check_record(name, rec, want, c):
    """Decisions exactly, figures within C * 2^-53 * max_dist -> the worst ratio of the three figures."""
    assert int(rec["status"]) == want["status"] and int(rec["n_query"]) == len(c["query"]), name
    assert (int(rec["n_matched"]), int(rec["worst"])) == (want["n_matched"], want["worst"]), name
    assert rec["n_within"].tolist() == want["n_within"].tolist() + [0] * (4 - len(want["n_within"])), name
    worst = 0.0
    for f in FIGURES:
        assert np.isnan(rec[f]) == np.isnan(want[f]), (name, f)
        if not np.isnan(want[f]):
            ratio = abs(float(rec[f]) - want[f]) / (cc.ULP * c["max_dist"])
            assert ratio <= cc.C, (name, f, ratio, float(rec[f]), want[f])
            worst = max(worst, ratio)
    return worst


def check_nn(name, idx, d2, b):
    assert np.array_equal(idx, b["j"]) and d2.tobytes() == b["d2"].tobytes(), name


def extras(names):
    """Pairs that share clouds.  In the large group: the 257-point query against three other references (the heavy cell among them), the 257-point
    reference under two other queries; elsewhere the first query against every reference of the group."""
    if "s257_257" not in names:
        return [(0, k) for k in range(1, len(names))]
    at = names.index
    return [(at("s257_257"), at(r)) for r in ("heavy_cell", "s64_65", "around_zero")] + [(at(q), at("s257_257")) for q in ("s65_63", "outside_xp")]


def test_every_case_in_one_call_and_alone(g, brute):
    worst = (0.0, None)
    for (max_dist, _), names in cc.groups().items():
        ex = extras(names)
        many = Call(g, names, ex)
        try:
            res, nn_off, idx, d2 = many.run()
        finally:
            many.free()
        for i, name in enumerate(names):
            c, a, b = cc.CASES[name], int(nn_off[i]), int(nn_off[i + 1])
            ratio = check_record(name, res[i], GOLDEN[name], c)
            if ratio > worst[0]:
                worst = (ratio, name)
            check_nn(name, idx[a:b], d2[a:b], brute[name])
            assert np.array_equal(idx[a:b], GOLDEN[name]["j"]) and np.array_equal(idx[a:b] != cc.NO_MATCH, GOLDEN[name]["matched"]), name
            alone = Call(g, [name])
            try:
                r1, _, i1, d1 = alone.run()
            finally:
                alone.free()
            assert r1[0].tobytes() == res[i].tobytes(), name        # a pair's record has the same bits whatever else the call holds
            assert np.array_equal(i1, idx[a:b]) and d1.tobytes() == d2[a:b].tobytes(), name
        for k, (qi, ri) in enumerate(ex, start=len(names)):          # the pairs across cases, against the brute force
            q, r = cc.CASES[names[qi]]["query"], cc.CASES[names[ri]]["ref"]
            want = cloudmetrics.c2c(q, r, max_dist, many.thr)
            a, b = int(nn_off[k]), int(nn_off[k + 1])
            check_nn((names[qi], names[ri]), idx[a:b], d2[a:b], want)
            assert (int(res[k]["status"]), int(res[k]["n_matched"]), int(res[k]["worst"])) == (want["status"], want["n_matched"], want["worst"])
            assert res[k]["n_within"][:len(many.thr)].tolist() == want["n_within"]
            for f in FIGURES:
                assert (np.isnan(res[k][f]) and np.isnan(want[f])) or abs(float(res[k][f]) - want[f]) <= 2 * cc.C * cc.ULP * max_dist, (names[qi], names[ri], f)
    print(f"\ndevice: worst ratio {worst[0]:.3f} at {worst[1]} (C {cc.C})")


def test_self_pair_is_exactly_zero(g):
    """A cloud against itself through ONE buffer on both sides: every d2 exactly 0.0, every figure exactly 0.0, j(i) = i but behind an earlier duplicate."""
    c = cc.CASES["self"]
    rec, off = side([c["query"]])
    gq = devguard.Guarded.input(g, rec, offset=16, name="c2c self")
    gi, gd = devguard.Guarded(g, 4 * 96, offset=4, name="c2c self idx"), devguard.Guarded(g, 8 * 96, offset=8, name="c2c self d2")
    try:
        res, _ = g.clouds_c2c_dev(gq.ptr, off, gq.ptr, off, [(0, 0)], c["max_dist"], c["thr"], gi.ptr, gd.ptr)
        gq.check()
        assert [float(res[0][f]) for f in FIGURES] == [0.0, 0.0, 0.0] and int(res[0]["n_matched"]) == 96 and res[0]["n_within"].tolist() == [96, 96, 96, 0]
        assert not gd.read(np.float64).any() and gi.read(np.uint32).tolist() == GOLDEN["self"]["j"].tolist()
    finally:
        gq.free(), gi.free(), gd.free()


@pytest.fixture(scope="module")
def main_group():
    return cc.groups()[(cc.M, np.asarray(cc.THR, dtype=np.float64).tobytes())]


def test_status_pairs_leave_their_neighbours_alone(g, main_group):
    """The group's call with and without the four non-finite cases: every other pair keeps its bits."""
    bad = ["nan_query", "inf_query", "nan_ref", "inf_ref"]
    assert all(n in main_group for n in bad)
    a = Call(g, main_group)
    b = Call(g, [n for n in main_group if n not in bad])
    try:
        ra, oa, ia, da = a.run()
        rb, ob, ib, db = b.run()
    finally:
        a.free(), b.free()
    keep = [i for i, n in enumerate(main_group) if n not in bad]
    assert ra[keep].tobytes() == rb.tobytes()
    assert np.array_equal(np.concatenate([ia[int(oa[i]):int(oa[i + 1])] for i in keep]), ib)
    for i, n in enumerate(main_group):
        if n in bad:
            r = ra[i]
            assert int(r["status"]) == abi.LK_C2C_NONFINITE and all(np.isnan(r[f]) for f in FIGURES) and int(r["n_query"]) == 20
            assert (int(r["n_matched"]), int(r["worst"]), r["n_within"].tolist()) == (0, 0, [0, 0, 0, 0])
            assert (ia[int(oa[i]):int(oa[i + 1])] == cc.NO_MATCH).all() and np.isposinf(da[int(oa[i]):int(oa[i + 1])]).all()
    # out of range: its own group (max_dist 2^-10)
    names = ["range_query", "range_ref", "range_edge_inside"]
    c = Call(g, names)
    try:
        r, o, i_, d_ = c.run()
    finally:
        c.free()
    assert r["status"].tolist() == [abi.LK_C2C_RANGE, abi.LK_C2C_RANGE, 0] and int(r[2]["n_matched"]) == 2 and np.isposinf(d_[:3]).all()


def test_null_nn_outputs_host_entry_and_poisoned_pools(g, hip_lib, main_group, clean_env):
    names, ex = main_group, extras(main_group)
    full = Call(g, names, ex)
    bare = Call(g, names, ex, with_nn=False)
    try:
        res, nn_off, idx, d2 = full.run()
        res0, nn_off0, _, _ = bare.run()
        assert res0.tobytes() == res.tobytes() and np.array_equal(nn_off0, nn_off)                 # NULL nn outputs: the same records
        hres, hoff, hidx, hd2 = g.clouds_c2c(full.q, full.qo, full.r, full.ro, full.pairs, full.max_dist, full.thr, want_nn=True)
        assert hres.tobytes() == res.tobytes() and np.array_equal(hoff, nn_off) and np.array_equal(hidx, idx) and hd2.tobytes() == d2.tobytes()
        hres2, _ = g.clouds_c2c(full.q, full.qo, full.r, full.ro, full.pairs, full.max_dist, full.thr)
        assert hres2.tobytes() == res.tobytes()
    finally:
        full.free(), bare.free()
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        for with_nn in (True, False):
            p = Call(gp, names, ex, with_nn=with_nn)
            try:
                pres, _, pidx, pd2 = p.run()
            finally:
                p.free()
            assert pres.tobytes() == res.tobytes()
            if with_nn:
                assert np.array_equal(pidx, idx) and pd2.tobytes() == d2.tobytes()
        assert gp.clouds_c2c(full.q, full.qo, full.r, full.ro, full.pairs, full.max_dist, full.thr)[0].tobytes() == res.tobytes()
    finally:
        gp.close()


def raw_call(g, fn, query, n_q, q_off, ref, n_r, r_off, n_pairs, pq, pr, max_dist, thr, n_thr, out, idx, d2, nn_off):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = fn(g.h, ptr(query), C.c_size_t(n_q), arr(q_off), ptr(ref), C.c_size_t(n_r), arr(r_off), C.c_size_t(n_pairs), arr(pq), arr(pr), C.c_double(max_dist),
             arr(thr), C.c_uint32(n_thr), arr(out), ptr(idx), ptr(d2), arr(nn_off))
    return rc_, g.L.lk_last_error(g.h).decode()


def test_refusals(g):
    names = ["s2_2", "s65_63", "dup_ref"]
    call = Call(g, names, [(0, 1)])
    good, good_off, good_idx, good_d2 = call.run()
    n = len(call.pairs)
    Q, R_, I, D = call.gq.ptr, call.gr.ptr, call.gi.ptr, call.gd.ptr
    pq, pr = np.ascontiguousarray(call.pairs[:, 0]), np.ascontiguousarray(call.pairs[:, 1])
    thr = np.asarray(cc.THR, dtype=np.float64)
    base = dict(query=Q, n_q=len(call.qo) - 1, q_off=call.qo, ref=R_, n_r=len(call.ro) - 1, r_off=call.ro, n_pairs=n, pq=pq, pr=pr, max_dist=cc.M, thr=thr, n_thr=3,
                idx=I, d2=D)
    dec_q, dec_r = call.qo.copy(), call.ro.copy()
    dec_q[1], dec_r[2] = dec_q[2] + 1, dec_r[1] - 1
    past_q, past_r = pq.copy(), pr.copy()
    past_q[1], past_r[2] = len(call.qo) - 1, 77
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                           # noqa: E731
    thr_of = lambda *v: np.array(v, dtype=np.float64)                                       # noqa: E731
    q_rec0 = Q + 16 * int(call.qo[0])
    refusals = [
        (dict(n_pairs=0), -1, "n_pairs"), (dict(query=None), -1, "null argument (query)"), (dict(ref=None), -1, "null argument (ref)"),
        (dict(q_off=None), -1, "null argument (q_off)"), (dict(r_off=None), -1, "null argument (r_off)"), (dict(pq=None), -1, "null argument (pair_q)"),
        (dict(pr=None), -1, "null argument (pair_r)"), (dict(out=None), -1, "null argument (out)"),
        (dict(d2=None), -1, "nn_idx without nn_d2"), (dict(idx=None), -1, "nn_d2 without nn_idx"), (dict(nn_off=None), -1, "need nn_off"),
        (dict(query=Q + 8), -1, "query must be 16-byte aligned"), (dict(ref=R_ + 4), -1, "ref must be 16-byte aligned"),
        (dict(idx=I + 2), -1, "nn_idx must be 4-byte aligned"), (dict(d2=D + 4), -1, "nn_d2 must be 8-byte aligned"),
        (dict(q_off=dec_q), -1, "q_off decreases at cloud 1"), (dict(r_off=dec_r), -1, "r_off decreases at cloud 1"),
        (dict(pq=past_q), -1, "pair_q[1] is past"), (dict(pr=past_r), -1, "pair_r[2] is past"),
        (dict(max_dist=0.0), -1, "max_dist"), (dict(max_dist=-1.0), -1, "max_dist"), (dict(max_dist=np.nan), -1, "max_dist"), (dict(max_dist=np.inf), -1, "max_dist"),
        (dict(n_thr=5), -1, "n_thr is 5"), (dict(thr=None), -1, "null argument (thr)"),
        (dict(thr=thr_of(0.05, np.nan, 0.25)), -1, "thr[1]"), (dict(thr=thr_of(-0.01, 0.1, 0.25)), -1, "thr[0]"),
        (dict(thr=thr_of(0.05, 0.1, np.nextafter(0.25, 1.0))), -1, "thr[2]"), (dict(thr=thr_of(0.05, np.inf, 0.25)), -1, "thr[1]"),
        (dict(idx=q_rec0 + 16), -1, "nn_idx overlaps an input cloud"), (dict(d2=R_ + 16 * int(call.ro[-1]) - 8), -1, "nn_d2 overlaps an input cloud"),
        (dict(idx=D + 8), -1, "nn_idx overlaps nn_d2"),
        (dict(r_off=u64(0, 1, 2, 3, 1 << 31), n_r=4), -3, "ref holds 2^31 records or more"),
        (dict(q_off=u64(0, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), n_q=4), -3, "query cloud 0 holds 2^32 - 1 records or more"),
        (dict(q_off=u64(0, 1 << 30, 2 << 30, 3 << 30, 4 << 30), n_q=4, pq=np.array([0, 1, 2, 3], dtype=np.uint32)), -3, "2^32 records or more in all"),
    ]
    try:
        for change, code, word in refusals:
            out = np.full(n + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
            nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(base, out=out, nn_off=nn_off)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_c2c_dev, **kw)
            assert rc_ == code and word in msg and "lk_clouds_c2c_dev: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)) and devguard.untouched(nn_off.view(np.uint8)), change   # a refused call writes nothing
            call.gq.check(), call.gr.check()
            assert call.gi.check().tobytes() == good_idx.tobytes() and call.gd.check().tobytes() == good_d2.tobytes(), change
            again = call.run()                                                       # the handle is usable, a good call is right
            assert again[0].tobytes() == good.tobytes() and again[3].tobytes() == good_d2.tobytes(), change
        # the host entry refuses the same way, under its own name (4-byte alignment for its clouds)
        hq, hr = np.ascontiguousarray(call.q), np.ascontiguousarray(call.r)
        hi, hd = np.zeros(call.total, dtype=np.uint32), np.zeros(call.total, dtype=np.float64)
        hbase = dict(base, query=hq.ctypes.data, ref=hr.ctypes.data, idx=hi.ctypes.data, d2=hd.ctypes.data)
        for change, code, word in ((dict(n_pairs=0), -1, "n_pairs"), (dict(max_dist=np.nan), -1, "max_dist"), (dict(query=hq.ctypes.data + 2), -1, "query must be 4-byte aligned"),
                                   (dict(idx=hq.ctypes.data + 16 * LEAD), -1, "nn_idx overlaps an input cloud"), (dict(r_off=u64(0, 1, 2, 3, 1 << 31), n_r=4), -3, "2^31")):
            out = np.full(n + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
            nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(hbase, out=out, nn_off=nn_off)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_c2c, **kw)
            assert rc_ == code and word in msg and "lk_clouds_c2c: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)) and devguard.untouched(nn_off.view(np.uint8)) and not hi.any() and not hd.any(), change
        # a good call writes every byte of its n_pairs records and nothing behind them; nn_off alone is accepted; n_thr = 0 takes a null thr
        out = np.full(n + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
        nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        rc_, msg = raw_call(g, g.L.lk_clouds_c2c_dev, **dict(base, out=out, nn_off=nn_off, idx=None, d2=None))
        assert rc_ == 0 and out[:n].tobytes() == good.tobytes() and devguard.untouched(out[n:].view(np.uint8)) and np.array_equal(nn_off, good_off), msg
        rc_, msg = raw_call(g, g.L.lk_clouds_c2c_dev, **dict(base, out=out, nn_off=None, idx=None, d2=None, thr=None, n_thr=0))
        assert rc_ == 0 and not out[:n]["n_within"].any() and np.array_equal(out[:n]["n_matched"], good["n_matched"]) and out[:n]["rmse"].tobytes() == good["rmse"].tobytes(), msg
    finally:
        call.free()


# ---- end to end: two runs replayed on the frozen map, their registered clouds downsampled, the map clouds scored against each other where they lie

@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def built():
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()


def test_from_a_replay(built, oracle_lib, hip_lib, scene_plain):
    c = trr.build_case("plain", built, oracle_lib, hip_lib, scene_plain)
    runs, tbs, xs = c["runs"][:2], c["tbs"][:2], c["xs"][:2]   # runs of 3 scans and of 1
    t = hip_lib.flatten_runs(runs, tbs)
    n = len(t["pts"])
    file_off, file_run = hip_lib.pcd_file_offsets(t["run_off"], t["scan_off"], 100)
    assert file_run.tolist() == [0, 1]
    g = trr.new_handle(hip_lib, c["sc"], c["blob"], 2)
    d_pts = g.device_malloc(t["pts"].nbytes)
    gw = devguard.Guarded(g, 16 * n, offset=16, name="c2c replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="c2c replay d_out")
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * 2))
        _, sbo = g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, tmc.LEAF, go.ptr)
        m = int(out_off[-1])
        assert not unf.any() and m > 100
        img = go.check().copy()
        clouds = np.frombuffer(img[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        a, b = clouds[:int(out_off[1]), :3], clouds[int(out_off[1]):, :3]
        B = int(sbo[-1])
        before = (g.batch_get_states(0, 2), trr.times_of(g, 2), g.runs_bucket_poses(0, B).tobytes(), g.map_export().copy())
        gi, gd = devguard.Guarded(g, 4 * (2 * len(a) + len(b)), offset=4, name="c2c replay idx"), devguard.Guarded(g, 8 * (2 * len(a) + len(b)), offset=8, name="c2c replay d2")
        try:
            res, nn_off = g.clouds_c2c_dev(go.ptr, out_off, go.ptr, out_off, [(0, 1), (1, 0), (0, 0)], 0.25, (0.05, 0.1), gi.ptr, gd.ptr)
            assert go.check().tobytes() == img.tobytes(), "the call changed the map clouds"
            idx, d2 = gi.read(np.uint32), gd.read(np.float64)
        finally:
            gi.free(), gd.free()
        assert nn_off.tolist() == [0, len(a), len(a) + len(b), 2 * len(a) + len(b)]
        for k, (q, r) in enumerate(((a, b), (b, a), (a, a))):
            want = cloudmetrics.c2c(q, r, 0.25, (0.05, 0.1))
            lo, hi = int(nn_off[k]), int(nn_off[k + 1])
            assert np.array_equal(idx[lo:hi], want["j"]) and d2[lo:hi].tobytes() == want["d2"].tobytes(), k
            assert (int(res[k]["status"]), int(res[k]["n_query"]), int(res[k]["n_matched"]), int(res[k]["worst"])) == (0, len(q), want["n_matched"], want["worst"]), k
            assert res[k]["n_within"].tolist() == want["n_within"] + [0, 0], k
            for f in FIGURES:
                assert abs(float(res[k][f]) - want[f]) <= 2 * cc.C * cc.ULP * 0.25, (k, f)   # (either side within tol of the truth)
        print(f"replay: map clouds of {len(a)} and {len(b)} points, matched {int(res[0]['n_matched'])} / {int(res[1]['n_matched'])}, rmse {float(res[0]['rmse']):.4f} m")
        assert int(res[2]["n_matched"]) == len(a) and [float(res[2][f]) for f in FIGURES] == [0.0, 0.0, 0.0]
        assert idx[int(nn_off[2]):].tolist() == list(range(len(a))) and not d2[int(nn_off[2]):].any()
        p, r_, f_ = cloudmetrics.fscore(res[0], res[1], 1)
        assert 0.0 <= f_ <= 1.0 and p == int(res[0]["n_within"][1]) / len(a)
        # the slots, the bucket table and the map are as they were
        after = (g.batch_get_states(0, 2), trr.times_of(g, 2), g.runs_bucket_poses(0, B).tobytes(), g.map_export())
        assert np.array_equal(after[0][0], before[0][0]) and np.array_equal(after[0][1], before[0][1]) and after[1] == before[1]
        assert after[2] == before[2] and np.array_equal(after[3], before[3])
    finally:
        g.device_free(d_pts)
        gw.free()
        go.free()
        g.close()
