"""-m gpu: lk_clouds_align_plane_dev / lk_clouds_align_plane (point-to-plane alignment of many pairs of clouds, the loop on the device) and
lk_clouds_normals_dev / lk_clouds_normals (per-point normals).

The cases are the frozen tables of tests/planecases.py, the expected values their 50-digit evaluation (tests/golden/plane_cases.npz): iters, status,
counts, n_used, worst, the final search's j(i) / matched flags, validity and n_i are compared exactly; T, the figures and the normals within the
tolerance derived there.  Every call's clouds and normals lie between the guard bands of tests/devguard.py at payload offset 16, behind three
leading records of NaN that belong to nobody and in front of one more cloud of NaN that no pair names (test_c2c_gpu.side).  The nn arrays and the
normals output are guarded outputs of exactly their size."""
import ctypes as C

import numpy as np
import pytest

import aligncases as ac
import devguard
import planecases as pc
import scenes
import test_c2c_gpu as tcg
import test_map_clouds as tmc
import test_overlay_runs as tor
import test_replay_runs as trr
from legkilo_amd import abi, cloudmetrics

pytestmark = pytest.mark.gpu

GOLDEN, NGOLDEN = pc.golden(), pc.golden_normals()
REC, PL, C2C, NREC = abi.align_dtype(), abi.align_plane_dtype(), abi.c2c_dtype(), abi.normals_dtype()
MAIN = (pc.M, np.asarray(pc.THR, dtype=np.float64).tobytes(), pc.MAX_ITER, pc.EPS_ROT, pc.EPS_TRANS)
NMAIN = (pc.N_RADIUS, pc.N_MIN_PTS, pc.N_MIN_PLAN)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("LEGKILO_POISON_POOLS", raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def g(hip_lib):
    h = tmc.new_handle(hip_lib)
    yield h
    h.close()


class Call:
    """Cases (names of the table, equal scalar arguments) as ONE call in guarded device memory: pair i = (query cloud i, reference cloud i), then
    `extra` pairs of cloud indices, which start from the identity.  T0 is NULL when no case of the call gives one."""

    def __init__(self, g, names, extra=(), with_nn=True):
        self.g, self.names = g, list(names)
        cs = [pc.CASES[n] for n in names]
        c0 = cs[0]
        self.max_dist, self.thr, self.max_iter, self.eps = c0["max_dist"], c0["thr"], c0["max_iter"], (c0["eps_rot"], c0["eps_trans"])
        assert all((c["max_dist"], c["max_iter"], c["eps_rot"], c["eps_trans"]) == (self.max_dist, self.max_iter) + self.eps for c in cs)
        self.q, self.qo = tcg.side([c["query"] for c in cs])
        self.r, self.ro = tcg.side([c["ref"] for c in cs])
        self.n, no = tcg.side([c["normals"] for c in cs])
        assert np.array_equal(no, self.ro)
        self.pairs = np.array([(i, i) for i in range(len(cs))] + list(extra), dtype=np.uint32).reshape(-1, 2)
        self.T0 = np.stack([c["T0"] for c in cs] + [ac.IDENTITY] * len(extra)) if any(c["has_T0"] for c in cs) else None
        self.total = int(sum(int(self.qo[a + 1] - self.qo[a]) for a, _ in self.pairs))
        tag = f"plane {names[0]} {len(names)} {len(extra)}"
        self.gq = devguard.Guarded.input(g, self.q, offset=16, name=tag + " query")
        self.gr = devguard.Guarded.input(g, self.r, offset=16, name=tag + " ref")
        self.gn = devguard.Guarded.input(g, self.n, offset=16, name=tag + " normals")
        self.gi = devguard.Guarded(g, 4 * self.total, offset=4, name=tag + " nn_idx") if with_nn else None
        self.gd = devguard.Guarded(g, 8 * self.total, offset=8, name=tag + " nn_d2") if with_nn else None

    def run(self, want_c2c=True):
        """-> (align records, plane records, lk_c2c records or None, nn_off, nn_idx, nn_d2); bands untouched, inputs unmodified."""
        out, pl, res, nn_off = self.g.clouds_align_plane_dev(self.gq.ptr, self.qo, self.gr.ptr, self.ro, self.gn.ptr, self.pairs, self.max_dist, self.T0, self.max_iter,
                                                             self.eps[0], self.eps[1], self.thr, self.gi.ptr if self.gi else 0, self.gd.ptr if self.gd else 0, want_c2c)
        self.gq.check(), self.gr.check(), self.gn.check()
        assert len(out) == len(pl) == len(self.pairs) and int(nn_off[0]) == 0 and int(nn_off[-1]) == self.total
        if not self.gi:
            return out, pl, res, nn_off, None, None
        idx, d2 = self.gi.read(np.uint32), self.gd.read(np.float64)
        assert len(idx) == len(d2) == self.total
        if self.total:
            assert devguard.sentinel_free(d2) and not np.isnan(d2).any()
        return out, pl, res, nn_off, idx, d2

    def free(self):
        for b in (self.gq, self.gr, self.gn, self.gi, self.gd):
            if b:
                b.free()


def as_got(a, p, c, idx=None):
    """One pair's three records (and its nn_idx slice) in the shape planecases.compare takes."""
    got = dict(T=np.r_[a["rot"], a["trans"]], iters=int(a["iters"]), status=int(a["status"]), n_matched_first=int(a["n_matched_first"]), rmse_first=float(a["rmse_first"]),
               step_rot=float(a["step_rot"]), step_trans=float(a["step_trans"]), rmse=float(c["rmse"]), mean=float(c["mean"]), max=float(c["max"]),
               n_matched=int(c["n_matched"]), n_within=c["n_within"].tolist(), worst=int(c["worst"]), rmse_plane_first=float(p["rmse_plane_first"]),
               rmse_plane=float(p["rmse_plane"]), n_used_first=int(p["n_used_first"]), n_used=int(p["n_used"]))
    if idx is not None:
        got.update(j=idx, matched=idx != pc.NO_MATCH)
    return got


def extras(names):
    """Pairs that share clouds, in the large group: a query against another case's reference and normals."""
    if "s255_257" not in names or "both" not in names:
        return []
    at = names.index
    return [(at("both"), at("s255_257")), (at("s257_255"), at("s255_257"))]


def test_every_case_in_one_call_and_alone(g):
    worst = dict(R=(0.0, ""), T=(0.0, ""), FIG=(0.0, ""))
    for key, names in pc.groups().items():
        ex = extras(names)
        many = Call(g, names, ex)
        try:
            out, pl, res, nn_off, idx, d2 = many.run()
        finally:
            many.free()
        for i, name in enumerate(names):
            c, a, b = pc.CASES[name], int(nn_off[i]), int(nn_off[i + 1])
            assert int(res[i]["n_query"]) == len(c["query"]) and int(res[i]["status"]) == (GOLDEN[name]["status"] & 3), name
            for k, v in pc.compare(name, as_got(out[i], pl[i], res[i], idx[a:b]), GOLDEN[name]).items():
                worst[k] = max(worst[k], (v, name))
            unmatched = idx[a:b] == pc.NO_MATCH
            assert np.isposinf(d2[a:b][unmatched]).all() and (d2[a:b][~unmatched] <= c["max_dist"] ** 2).all(), name
            alone = Call(g, [name])
            try:
                o1, p1, r1, _, i1, d1 = alone.run()
            finally:
                alone.free()
            assert o1[0].tobytes() == out[i].tobytes() and p1[0].tobytes() == pl[i].tobytes() and r1[0].tobytes() == res[i].tobytes(), name   # the same bits whatever else the call holds
            assert np.array_equal(i1, idx[a:b]) and d1.tobytes() == d2[a:b].tobytes(), name
        for k, (qi, ri) in enumerate(ex, start=len(names)):          # the pairs across cases, against the numpy statement
            q, r, nr = pc.CASES[names[qi]]["query"], pc.CASES[names[ri]]["ref"], pc.CASES[names[ri]]["normals"]
            want = cloudmetrics.align_plane(q, r, nr, many.max_dist, None, many.max_iter, many.eps[0], many.eps[1], many.thr)
            assert (int(out[k]["iters"]), int(out[k]["status"]), int(pl[k]["n_used_first"]), int(pl[k]["n_used"])) == (want["iters"], want["status"], want["n_used_first"],
                                                                                                                     want["n_used"]), (qi, ri)
            a, b = int(nn_off[k]), int(nn_off[k + 1])
            assert np.array_equal(idx[a:b], want["c2c"]["j"]) and int(res[k]["n_matched"]) == want["c2c"]["n_matched"], (qi, ri)
            T = np.r_[out[k]["rot"], out[k]["trans"]]
            assert np.abs(T[:9] - want["T"][:9]).max() <= 2 * pc.C_R * pc.ULP and np.abs(T[9:] - want["T"][9:]).max() <= 2 * pc.C_T * pc.ULP * 2.5, (qi, ri)
    print(f"\ndevice: worst ratios {worst} (C {pc.C_R}, {pc.C_T}, {pc.C_FIG})")


def test_optional_outputs_host_entry_and_poisoned_pools(g, hip_lib, clean_env):
    names = pc.groups()[MAIN]
    ex = extras(names)
    full, bare = Call(g, names, ex), Call(g, names, ex, with_nn=False)
    args = lambda c: (c.q, c.qo, c.r, c.ro, c.n, c.pairs, c.max_dist, c.T0, c.max_iter, c.eps[0], c.eps[1], c.thr)   # noqa: E731
    try:
        out, pl, res, nn_off, idx, d2 = full.run()
        o0, p0, r0, off0, _, _ = bare.run()
        assert o0.tobytes() == out.tobytes() and p0.tobytes() == pl.tobytes() and r0.tobytes() == res.tobytes() and np.array_equal(off0, nn_off)   # NULL nn outputs
        o1, p1, r1, _, i1, d1 = full.run(want_c2c=False)
        assert r1 is None and o1.tobytes() == out.tobytes() and p1.tobytes() == pl.tobytes() and np.array_equal(i1, idx) and d1.tobytes() == d2.tobytes()   # NULL c2c_out
        # NULL pl_out: the same lk_align records
        n = len(full.pairs)
        o2 = np.zeros(n, dtype=REC)
        pq, pr = np.ascontiguousarray(full.pairs[:, 0]), np.ascontiguousarray(full.pairs[:, 1])
        rc_, msg = raw_call(g, g.L.lk_clouds_align_plane_dev, query=full.gq.ptr, n_q=len(full.qo) - 1, q_off=full.qo, ref=full.gr.ptr, n_r=len(full.ro) - 1, r_off=full.ro,
                            n_pairs=n, pq=pq, pr=pr, max_dist=full.max_dist, thr=full.thr, n_thr=len(full.thr), T0=full.T0, max_iter=full.max_iter, eps_rot=full.eps[0],
                            eps_trans=full.eps[1], normals=full.gn.ptr, out=o2, pl=None, c2c=None, idx=None, d2=None, nn_off=None)
        assert rc_ == 0 and o2.tobytes() == out.tobytes(), msg
        ho, hp, hr, hoff, hidx, hd2 = g.clouds_align_plane(*args(full), want_nn=True)
        assert ho.tobytes() == out.tobytes() and hp.tobytes() == pl.tobytes() and hr.tobytes() == res.tobytes() and np.array_equal(hoff, nn_off)
        assert np.array_equal(hidx, idx) and hd2.tobytes() == d2.tobytes()
        ho2, hp2, hr2, _ = g.clouds_align_plane(*args(full))
        assert ho2.tobytes() == out.tobytes() and hp2.tobytes() == pl.tobytes() and hr2.tobytes() == res.tobytes()
    finally:
        full.free(), bare.free()
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        p = Call(gp, names, ex)
        try:
            po, pp, pr_, _, pidx, pd2 = p.run()
        finally:
            p.free()
        assert po.tobytes() == out.tobytes() and pp.tobytes() == pl.tobytes() and pr_.tobytes() == res.tobytes() and np.array_equal(pidx, idx) and pd2.tobytes() == d2.tobytes()
        ho, hp, hr, _ = gp.clouds_align_plane(*args(full))
        assert ho.tobytes() == out.tobytes() and hp.tobytes() == pl.tobytes() and hr.tobytes() == res.tobytes()
    finally:
        gp.close()


def test_status_pairs_leave_their_neighbours_alone(g):
    names = pc.groups()[MAIN]
    bad = ["nan_query", "nan_ref", "range_query", "bad_t0"]
    assert all(n in names for n in bad)
    a, b = Call(g, names), Call(g, [n for n in names if n not in bad])
    try:
        oa, pa, ra, offa, ia, da = a.run()
        ob, pb, rb, _, ib, _ = b.run()
    finally:
        a.free(), b.free()
    keep = [i for i, n in enumerate(names) if n not in bad]
    assert oa[keep].tobytes() == ob.tobytes() and pa[keep].tobytes() == pb.tobytes() and ra[keep].tobytes() == rb.tobytes()
    assert np.array_equal(np.concatenate([ia[int(offa[i]):int(offa[i + 1])] for i in keep]), ib)
    for i, n in enumerate(names):
        if n in bad:
            r, c = oa[i], pc.CASES[n]
            assert int(r["status"]) == GOLDEN[n]["status"] and np.r_[r["rot"], r["trans"]].tobytes() == c["T0"].tobytes(), n
            assert (int(r["iters"]), int(r["n_matched_first"])) == (0, 0) and all(np.isnan(r[f]) for f in ("rmse_first", "step_rot", "step_trans")), n
            assert np.isnan(pa[i]["rmse_plane_first"]) and np.isnan(pa[i]["rmse_plane"]) and (int(pa[i]["n_used_first"]), int(pa[i]["n_used"])) == (0, 0), n
            assert (ia[int(offa[i]):int(offa[i + 1])] == pc.NO_MATCH).all() and np.isposinf(da[int(offa[i]):int(offa[i + 1])]).all(), n
            assert int(ra[i]["n_matched"]) == 0 and np.isnan(ra[i]["rmse"]) and int(ra[i]["n_query"]) == 20, n


def raw_call(g, fn, query, n_q, q_off, ref, n_r, r_off, n_pairs, pq, pr, max_dist, thr, n_thr, T0, max_iter, eps_rot, eps_trans, normals, out, pl, c2c, idx, d2, nn_off):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = fn(g.h, ptr(query), C.c_size_t(n_q), arr(q_off), ptr(ref), C.c_size_t(n_r), arr(r_off), C.c_size_t(n_pairs), arr(pq), arr(pr), C.c_double(max_dist),
             arr(thr), C.c_uint32(n_thr), arr(T0), C.c_uint32(max_iter), C.c_double(eps_rot), C.c_double(eps_trans), ptr(normals), arr(out), arr(pl), arr(c2c), ptr(idx),
             ptr(d2), arr(nn_off))
    return rc_, g.L.lk_last_error(g.h).decode()


def test_refusals(g):
    names = ["s6_65", "both", "t0_answer"]
    call = Call(g, names, [(0, 1)])
    good, good_p, good_c, good_off, good_idx, good_d2 = call.run()
    n = len(call.pairs)
    Q, R_, N_, I, D = call.gq.ptr, call.gr.ptr, call.gn.ptr, call.gi.ptr, call.gd.ptr
    pq, pr = np.ascontiguousarray(call.pairs[:, 0]), np.ascontiguousarray(call.pairs[:, 1])
    thr = np.asarray(pc.THR, dtype=np.float64)
    T0 = np.ascontiguousarray(call.T0)
    base = dict(query=Q, n_q=len(call.qo) - 1, q_off=call.qo, ref=R_, n_r=len(call.ro) - 1, r_off=call.ro, n_pairs=n, pq=pq, pr=pr, max_dist=pc.M, thr=thr, n_thr=3,
                T0=T0, max_iter=pc.MAX_ITER, eps_rot=pc.EPS_ROT, eps_trans=pc.EPS_TRANS, normals=N_, idx=I, d2=D)
    dec_q = call.qo.copy()
    dec_q[1] = dec_q[2] + 1
    past_r = pr.copy()
    past_r[2] = 77
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                           # noqa: E731
    n_rec0 = N_ + 16 * int(call.ro[0])
    refusals = [
        # refusals of lk_clouds_c2c_dev and lk_clouds_align_dev, through the shared checks
        (dict(n_pairs=0), -1, "n_pairs"), (dict(query=None), -1, "null argument (query)"), (dict(ref=None), -1, "null argument (ref)"),
        (dict(q_off=None), -1, "null argument (q_off)"), (dict(pr=None), -1, "null argument (pair_r)"), (dict(d2=None), -1, "nn_idx without nn_d2"),
        (dict(nn_off=None), -1, "need nn_off"), (dict(query=Q + 8), -1, "query must be 16-byte aligned"), (dict(idx=I + 2), -1, "nn_idx must be 4-byte aligned"),
        (dict(q_off=dec_q), -1, "q_off decreases at cloud 1"), (dict(pr=past_r), -1, "pair_r[2] is past"), (dict(max_dist=np.nan), -1, "max_dist"),
        (dict(n_thr=5), -1, "n_thr is 5"), (dict(idx=Q + 16 * int(call.qo[0]) + 16), -1, "nn_idx overlaps an input cloud"), (dict(idx=D + 8), -1, "nn_idx overlaps nn_d2"),
        (dict(r_off=u64(0, 1, 2, 3, 1 << 31), n_r=4), -3, "ref holds 2^31 records or more"),
        (dict(out=None), -1, "null argument (out)"), (dict(max_iter=1001), -1, "max_iter is 1001"), (dict(eps_rot=np.nan), -1, "eps_rot"), (dict(eps_trans=-1.0), -1, "eps_trans"),
        # and its own
        (dict(normals=None), -1, "null argument (ref_normals)"), (dict(normals=N_ + 8), -1, "ref_normals must be 16-byte aligned"),
        (dict(idx=n_rec0 + 16), -1, "nn_idx overlaps ref_normals"), (dict(d2=N_ + 16 * int(call.ro[-1]) - 8), -1, "nn_d2 overlaps ref_normals"),
    ]
    fresh = lambda dt, k: np.full(k, 0xFF, dtype=np.uint8).repeat(dt.itemsize).view(dt)      # noqa: E731
    try:
        for change, code, word in refusals:
            out, pl, c2c = fresh(REC, n + 2), fresh(PL, n + 2), fresh(C2C, n + 2)
            nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(base, out=out, pl=pl, c2c=c2c, nn_off=nn_off)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_align_plane_dev, **kw)
            assert rc_ == code and word in msg and "lk_clouds_align_plane_dev: " in msg, (change, rc_, msg)
            assert all(devguard.untouched(x.view(np.uint8)) for x in (out, pl, c2c, nn_off)), change
            call.gq.check(), call.gr.check(), call.gn.check()
            assert call.gi.check().tobytes() == good_idx.tobytes() and call.gd.check().tobytes() == good_d2.tobytes(), change
        again = call.run()                                                           # the handle is usable, a good call is right
        assert again[0].tobytes() == good.tobytes() and again[1].tobytes() == good_p.tobytes() and again[2].tobytes() == good_c.tobytes() and again[5].tobytes() == good_d2.tobytes()
        # the host entry refuses the same way, under its own name (4-byte alignment)
        hq, hr, hn = np.ascontiguousarray(call.q), np.ascontiguousarray(call.r), np.ascontiguousarray(call.n)
        hi, hd = np.zeros(call.total, dtype=np.uint32), np.zeros(call.total, dtype=np.float64)
        hbase = dict(base, query=hq.ctypes.data, ref=hr.ctypes.data, normals=hn.ctypes.data, idx=hi.ctypes.data, d2=hd.ctypes.data)
        for change, code, word in ((dict(n_pairs=0), -1, "n_pairs"), (dict(max_iter=1001), -1, "max_iter"), (dict(normals=None), -1, "null argument (ref_normals)"),
                                   (dict(normals=hn.ctypes.data + 2), -1, "ref_normals must be 4-byte aligned"), (dict(out=None), -1, "null argument (out)")):
            out, pl, c2c = fresh(REC, n + 2), fresh(PL, n + 2), fresh(C2C, n + 2)
            nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(hbase, out=out, pl=pl, c2c=c2c, nn_off=nn_off)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_align_plane, **kw)
            assert rc_ == code and word in msg and "lk_clouds_align_plane: " in msg, (change, rc_, msg)
            assert all(devguard.untouched(x.view(np.uint8)) for x in (out, pl, c2c, nn_off)) and not hi.any() and not hd.any(), change
        # a good call writes every byte of its n_pairs records and nothing behind them; max_iter 1000 and eps 0 are accepted and leave R a rotation
        out, pl, c2c = fresh(REC, n + 2), fresh(PL, n + 2), fresh(C2C, n + 2)
        nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        rc_, msg = raw_call(g, g.L.lk_clouds_align_plane_dev, **dict(base, out=out, pl=pl, c2c=c2c, nn_off=nn_off, idx=None, d2=None))
        assert rc_ == 0 and out[:n].tobytes() == good.tobytes() and pl[:n].tobytes() == good_p.tobytes() and c2c[:n].tobytes() == good_c.tobytes(), msg
        assert np.array_equal(nn_off, good_off) and all(devguard.untouched(x[n:].view(np.uint8)) for x in (out, pl, c2c))
        rc_, msg = raw_call(g, g.L.lk_clouds_align_plane_dev, **dict(base, out=out, pl=pl, c2c=None, nn_off=None, idx=None, d2=None, thr=None, n_thr=0, T0=None,
                                                                      max_iter=1000, eps_rot=0.0, eps_trans=0.0))
        assert rc_ == 0 and all(ac.is_rotation(out[k]["rot"], 16.0) for k in range(3)) and (out[:3]["iters"] >= 3).all() and (pl[:3]["rmse_plane"] < 1e-8).all(), msg
    finally:
        call.free()


# ---- lk_clouds_normals_dev

class NCall:
    """Normals cases (equal scalar arguments) as ONE call: the clouds in guarded device memory, the records a guarded output of exactly their size."""

    def __init__(self, g, names):
        self.g, self.names = g, list(names)
        c0 = pc.NCASES[names[0]]
        self.args = (c0["radius"], c0["min_pts"], c0["min_planarity"])
        self.rec, self.off = tcg.side([pc.NCASES[n]["cloud"] for n in names])
        self.total = int(self.off[-1] - self.off[0])
        self.gc = devguard.Guarded.input(g, self.rec, offset=16, name=f"normals {names[0]} clouds")
        self.go = devguard.Guarded(g, 16 * self.total, offset=16, name=f"normals {names[0]} out")

    def run(self):
        res = self.g.clouds_normals_dev(self.gc.ptr, self.off, self.args[0], self.go.ptr, self.args[1], self.args[2])
        self.gc.check()
        return res, self.go.read(np.float32).reshape(-1, 4)

    def free(self):
        self.gc.free(), self.go.free()


def test_normals_every_case_in_one_call_alone_host_entry_and_poisoned_pools(g, hip_lib, clean_env):
    worst, kept = dict(N=(0.0, ""), W=(0.0, "")), None
    for key, names in pc.ngroups().items():
        many = NCall(g, names)
        try:
            res, rec = many.run()
            rel = (many.off - many.off[0]).astype(np.int64)
            assert len(res) == len(names) + 1 and int(res[-1]["status"]) == 1 and np.isnan(rec[rel[-2]:]).all()        # the trailing cloud of NaN
            for i, name in enumerate(names):
                mine = rec[rel[i]:rel[i + 1]]
                assert int(res[i]["n_points"]) == len(pc.NCASES[name]["cloud"]) and int(res[i]["pad"]) == 0, name
                for k, v in pc.compare_normals(name, mine, None, NGOLDEN[name], int(res[i]["n_valid"]), int(res[i]["status"])).items():
                    worst[k] = max(worst[k], (v, name))
                if int(res[i]["status"]):
                    assert np.isnan(mine).all(), name
                alone = NCall(g, [name])
                try:
                    r1, rec1 = alone.run()
                finally:
                    alone.free()
                assert r1[0].tobytes() == res[i].tobytes() and rec1[:len(mine)].tobytes() == mine.tobytes(), name      # the same bits whatever else the call holds
            hres, hrec = g.clouds_normals(many.rec, many.off, *many.args)
            assert hres.tobytes() == res.tobytes() and hrec.tobytes() == rec.tobytes(), key
            if key == NMAIN:
                kept = (names, many.rec, many.off, many.args, res.copy(), rec.copy())
        finally:
            many.free()
    print(f"\ndevice normals: worst ratios {worst} (C {pc.C_N}, {pc.C_W})")
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        p = NCall(gp, kept[0])
        try:
            pres, prec = p.run()
        finally:
            p.free()
        assert pres.tobytes() == kept[4].tobytes() and prec.tobytes() == kept[5].tobytes()
    finally:
        gp.close()


def test_normals_are_consistent_with_mme_on_the_same_clouds(g):
    """n_i is lk_clouds_mme_dev's d_n, so with min_planarity 0 a point is valid exactly where d_n >= min_pts, and n_valid is that count."""
    names = pc.ngroups()[NMAIN]
    call = NCall(g, names)
    gn = devguard.Guarded(g, 4 * call.total, offset=4, name="normals mme d_n")
    try:
        res = g.clouds_normals_dev(call.gc.ptr, call.off, pc.N_RADIUS, call.go.ptr, pc.N_MIN_PTS, 0.0)
        rec = call.go.read(np.float32).reshape(-1, 4)
        mres = g.clouds_mme_dev(call.gc.ptr, call.off, pc.N_RADIUS, pc.N_MIN_PTS, d_n=gn.ptr)
        cnt = gn.read(np.uint32)
        rel = (call.off - call.off[0]).astype(np.int64)
        for i in range(len(res)):
            a, b = rel[i], rel[i + 1]
            dense = cnt[a:b] >= pc.N_MIN_PTS
            assert np.array_equal(~np.isnan(rec[a:b, 0]), dense) and np.array_equal(~np.isnan(rec[a:b, 3]), dense), i
            assert int(res[i]["n_valid"]) == int(dense.sum()) == int(mres[i]["n_dense"]) and int(res[i]["status"]) == int(mres[i]["status"]), i
            assert int(res[i]["n_points"]) == int(mres[i]["n_points"]), i
        assert int(res["n_valid"].sum()) > 500
    finally:
        call.free(), gn.free()


def test_normals_refusals(g):
    call = NCall(g, ["plane", "corner"])
    good_res, good = call.run()
    fn = g.L.lk_clouds_normals_dev
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    nc = len(call.off) - 1
    dec = call.off.copy()
    dec[1] = dec[2] + 1
    first = call.gc.ptr + 16 * int(call.off[0])
    base = dict(clouds=call.gc.ptr, n=nc, off=call.off, radius=pc.N_RADIUS, min_pts=5, min_planarity=0.3, normals=call.go.ptr)
    fresh = lambda k: np.full(k, 0xFF, dtype=np.uint8).repeat(NREC.itemsize).view(NREC)      # noqa: E731
    try:
        for change, code, word in [(dict(n=0), -1, "n_clouds is 0"), (dict(clouds=None), -1, "null argument (clouds)"), (dict(off=None), -1, "null argument (off)"),
                                   (dict(out=None), -1, "null argument (out)"), (dict(clouds=call.gc.ptr + 4), -1, "clouds must be 16-byte aligned"),
                                   (dict(off=dec), -1, "off decreases at cloud 1"), (dict(radius=0.0), -1, "radius"), (dict(radius=np.nan), -1, "radius"),
                                   (dict(min_pts=2), -1, "min_pts is 2"), (dict(min_pts=0), -1, "min_pts is 0"),
                                   (dict(min_planarity=np.nan), -1, "min_planarity"), (dict(min_planarity=-0.01), -1, "min_planarity"),
                                   (dict(min_planarity=np.nextafter(1.0, 2.0)), -1, "min_planarity"), (dict(min_planarity=np.inf), -1, "min_planarity"),
                                   (dict(normals=None), -1, "null argument (normals)"), (dict(normals=call.go.ptr + 8), -1, "normals must be 16-byte aligned"),
                                   (dict(normals=first + 16), -1, "normals overlaps the input clouds"), (dict(normals=first - 16), -1, "normals overlaps the input clouds"),
                                   (dict(off=np.array([0, 1 << 31], dtype=np.uint64), n=1), -3, "2^31 records or more")]:
            out = fresh(nc + 2)
            kw = dict(base, out=out)
            kw.update(change)
            rc_ = fn(g.h, ptr(kw["clouds"]), C.c_size_t(kw["n"]), arr(kw["off"]), C.c_double(kw["radius"]), C.c_uint32(kw["min_pts"]), C.c_double(kw["min_planarity"]),
                     arr(kw["out"]), ptr(kw["normals"]))
            msg = g.L.lk_last_error(g.h).decode()
            assert rc_ == code and word in msg and "lk_clouds_normals_dev: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)), change
            call.gc.check()
            assert call.go.check().tobytes() == good.tobytes(), change
        out = fresh(nc + 2)                                                                  # min_pts 3 and the ends of [0, 1] are accepted; nothing behind the records
        for mp_, pl_ in ((3, 0.0), (5, 1.0)):
            rc_ = fn(g.h, ptr(call.gc.ptr), C.c_size_t(nc), arr(call.off), C.c_double(pc.N_RADIUS), C.c_uint32(mp_), C.c_double(pl_), arr(out), ptr(call.go.ptr))
            assert rc_ == 0 and devguard.untouched(out[nc:].view(np.uint8)), g.L.lk_last_error(g.h).decode()
        res, rec = call.run()                                                                # the handle is usable, a good call is right
        assert res.tobytes() == good_res.tobytes() and rec.tobytes() == good.tobytes()
    finally:
        call.free()


# ---- end to end: a run replayed on the frozen map, its registered cloud downsampled, moved by a known T and aligned back with normals from entry 1

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
    runs, tbs, xs = c["runs"][:2], c["tbs"][:2], c["xs"][:2]
    t = hip_lib.flatten_runs(runs, tbs)
    n = len(t["pts"])
    file_off, _ = hip_lib.pcd_file_offsets(t["run_off"], t["scan_off"], 100)
    g = trr.new_handle(hip_lib, c["sc"], c["blob"], 2)
    d_pts = g.device_malloc(t["pts"].nbytes)
    gw = devguard.Guarded(g, 16 * n, offset=16, name="plane replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="plane replay d_out")
    gm = devguard.Guarded(g, 16 * n, offset=16, name="plane replay moved")
    gn = devguard.Guarded(g, 16 * n, offset=16, name="plane replay normals")
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * 2))
        g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, tmc.LEAF, go.ptr)
        m = int(out_off[-1])
        assert not unf.any() and m > 100
        img = go.check().copy()
        clouds = np.frombuffer(img[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        a_len = int(out_off[1])
        centre = clouds[:a_len, :3].astype(np.float64).mean(0)
        known = np.stack([ac.about(ac.rot(2, 0.8) @ ac.rot(0, -0.5), np.array([0.02, -0.015, 0.01]), centre), ac.IDENTITY])
        radius = 4.0 * tmc.LEAF
        nres = g.clouds_normals_dev(go.ptr, out_off, radius, gn.ptr, 5, 0.2)
        normals = np.frombuffer(gn.check()[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        want_n = cloudmetrics.normals(clouds[:a_len], radius, 5, 0.2)
        assert int(nres[0]["n_valid"]) == want_n["n_valid"] and np.array_equal(np.isnan(normals[:a_len, 0]), ~want_n["valid"])
        v = want_n["valid"]
        assert v.sum() >= 6 and pc.angle(normals[:a_len][v, :3], want_n["vec"][v]).max() <= pc.C_N * pc.ULP32
        g.clouds_transform_dev(go.ptr, out_off, known, gm.ptr)                                # cloud 0 moved by a known T, cloud 1 as it is
        moved = np.frombuffer(gm.check()[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        args = (0.25, None, 30, 1e-7, 1e-7, (0.05, 0.1))
        out, pl, res, _ = g.clouds_align_plane_dev(gm.ptr, out_off, go.ptr, out_off, gn.ptr, [(0, 0), (1, 1)], *args)
        p2p, p2p_res, _ = g.clouds_align_dev(gm.ptr, out_off, go.ptr, out_off, [(0, 0), (1, 1)], *args)
        assert go.check().tobytes() == img.tobytes() and gn.check()[:16 * m].tobytes() == normals.tobytes(), "the call changed its inputs"
        want = cloudmetrics.align_plane(moved[:a_len], clouds[:a_len], normals[:a_len], *args)
        L = float(np.abs(clouds[:a_len, :3]).max())
        T = np.r_[out[0]["rot"], out[0]["trans"]]
        assert (int(out[0]["iters"]), int(out[0]["status"]), int(out[0]["n_matched_first"])) == (want["iters"], want["status"], want["n_matched_first"])
        assert (int(pl[0]["n_used_first"]), int(pl[0]["n_used"]), int(res[0]["n_matched"])) == (want["n_used_first"], want["n_used"], want["c2c"]["n_matched"])
        assert np.abs(T[:9] - want["T"][:9]).max() <= 2 * pc.C_R * pc.ULP and np.abs(T[9:] - want["T"][9:]).max() <= 2 * pc.C_T * pc.ULP * L   # (either side within tol of the truth)
        assert abs(float(pl[0]["rmse_plane"]) - want["rmse_plane"]) <= 2 * pc.C_FIG * pc.ULP * 0.25
        print(f"\nreplay: map cloud of {a_len} points ({int(pl[0]['n_used'])} with a plane) moved and aligned back: point-to-plane {int(out[0]['iters'])} solves, status "
              f"{int(out[0]['status'])}, plane rmse {float(pl[0]['rmse_plane_first']):.4f} -> {float(pl[0]['rmse_plane']):.2e} m, rmse -> {float(res[0]['rmse']):.2e} m; "
              f"point-to-point {int(p2p[0]['iters'])} solves, status {int(p2p[0]['status'])}, rmse -> {float(p2p_res[0]['rmse']):.2e} m")
        if int(out[0]["status"]) == abi.LK_ALIGN_CONVERGED:                                   # aligned back: T undoes the known motion up to the float32 rounding of the moved cloud
            back = T[:9].reshape(3, 3)
            Rk, tk = known[0][:9].reshape(3, 3), known[0][9:]
            assert np.abs(back @ Rk - np.eye(3)).max() < 1e-5 and np.abs(back @ tk + T[9:]).max() < 1e-3
            assert float(pl[0]["rmse_plane"]) < 1e-4 < float(pl[0]["rmse_plane_first"])
        else:
            assert int(out[0]["status"]) & (abi.LK_ALIGN_DEGENERATE | abi.LK_ALIGN_FEW) or int(out[0]["iters"]) == 30
    finally:
        g.device_free(d_pts)
        gw.free(), go.free(), gm.free(), gn.free()
        g.close()
