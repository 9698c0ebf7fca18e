"""-m gpu: lk_clouds_align_dev / lk_clouds_align / lk_clouds_transform_dev - rigid alignment of many pairs of clouds, the loop on the device.

The cases are the frozen table of tests/aligncases.py, the expected values its 50-digit evaluation (tests/golden/align_cases.npz): iters, status,
counts, worst and the final search's j(i) / matched flags are compared exactly, T and the figures within the tolerance derived there
(aligncases.compare).  Every call's clouds lie between the guard bands of tests/devguard.py at payload offset 16, behind three leading records of
NaN that belong to nobody and in front of one more cloud of NaN that no pair names; every record's w is NaN (test_c2c_gpu.side).  The nn arrays are
guarded outputs of exactly nn_off[n_pairs] entries."""
import ctypes as C

import numpy as np
import pytest

import aligncases as ac
import devguard
import scenes
import test_c2c_gpu as tcg
import test_map_clouds as tmc
import test_overlay_runs as tor
import test_replay_runs as trr
from legkilo_amd import abi, cloudmetrics

pytestmark = pytest.mark.gpu

GOLDEN = ac.golden()
REC, C2C = abi.align_dtype(), abi.c2c_dtype()
MAIN = (ac.M, np.asarray(ac.THR, dtype=np.float64).tobytes(), ac.MAX_ITER, ac.EPS_ROT, ac.EPS_TRANS)


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
        cs = [ac.CASES[n] for n in names]
        c0 = cs[0]
        self.max_dist, self.thr, self.max_iter, self.eps = c0["max_dist"], c0["thr"], c0["max_iter"], (c0["eps_rot"], c0["eps_trans"])
        assert all((c["max_dist"], c["max_iter"], c["eps_rot"], c["eps_trans"]) == (self.max_dist, self.max_iter) + self.eps for c in cs)
        self.q, self.qo = tcg.side([c["query"] for c in cs])
        self.r, self.ro = tcg.side([c["ref"] for c in cs])
        self.pairs = np.array([(i, i) for i in range(len(cs))] + list(extra), dtype=np.uint32).reshape(-1, 2)
        self.T0 = np.stack([c["T0"] for c in cs] + [ac.IDENTITY] * len(extra)) if any(c["has_T0"] for c in cs) else None
        self.total = int(sum(int(self.qo[a + 1] - self.qo[a]) for a, _ in self.pairs))
        tag = f"align {names[0]} {len(names)} {len(extra)}"
        self.gq = devguard.Guarded.input(g, self.q, offset=16, name=tag + " query")
        self.gr = devguard.Guarded.input(g, self.r, offset=16, name=tag + " ref")
        self.gi = devguard.Guarded(g, 4 * self.total, offset=4, name=tag + " nn_idx") if with_nn else None
        self.gd = devguard.Guarded(g, 8 * self.total, offset=8, name=tag + " nn_d2") if with_nn else None

    def run(self, want_c2c=True):
        """-> (align records, lk_c2c records or None, nn_off, nn_idx, nn_d2); bands untouched, inputs unmodified."""
        out, res, nn_off = self.g.clouds_align_dev(self.gq.ptr, self.qo, self.gr.ptr, self.ro, self.pairs, self.max_dist, self.T0, self.max_iter, self.eps[0],
                                                   self.eps[1], self.thr, self.gi.ptr if self.gi else 0, self.gd.ptr if self.gd else 0, want_c2c)
        self.gq.check(), self.gr.check()
        assert len(out) == len(self.pairs) and int(nn_off[0]) == 0 and int(nn_off[-1]) == self.total
        assert np.array_equal(np.diff(nn_off.astype(np.int64)), [int(self.qo[a + 1] - self.qo[a]) for a, _ in self.pairs])
        if not self.gi:
            return out, res, nn_off, None, None
        idx, d2 = self.gi.read(np.uint32), self.gd.read(np.float64)
        assert len(idx) == len(d2) == self.total
        if self.total:
            assert devguard.sentinel_free(d2) and not np.isnan(d2).any()
        return out, res, nn_off, idx, d2

    def free(self):
        for b in (self.gq, self.gr, self.gi, self.gd):
            if b:
                b.free()


def as_got(a, c, idx=None):
    """One pair's two records (and its nn_idx slice) in the shape aligncases.compare takes."""
    got = dict(T=np.r_[a["rot"], a["trans"]], iters=int(a["iters"]), status=int(a["status"]), n_matched_first=int(a["n_matched_first"]), rmse_first=float(a["rmse_first"]),
               step_rot=float(a["step_rot"]), step_trans=float(a["step_trans"]), rmse=float(c["rmse"]), mean=float(c["mean"]), max=float(c["max"]),
               n_matched=int(c["n_matched"]), n_within=c["n_within"].tolist(), worst=int(c["worst"]))
    if idx is not None:
        got.update(j=idx, matched=idx != ac.NO_MATCH)
    return got


def extras(names):
    """Pairs that share clouds, in the large group: two queries against another case's reference, one reference under another query."""
    if "s64_65" not in names or "s63_64" not in names:
        return []
    at = names.index
    return [(at("s64_65"), at("s63_64")), (at("s257_255"), at("s256_256")), (at("both"), at("s256_256"))]


def test_every_case_in_one_call_and_alone(g):
    worst = dict(R=(0.0, None), T=(0.0, None), FIG=(0.0, None))
    for key, names in ac.groups().items():
        ex = extras(names)
        many = Call(g, names, ex)
        try:
            out, res, nn_off, idx, d2 = many.run()
        finally:
            many.free()
        for i, name in enumerate(names):
            c, a, b = ac.CASES[name], int(nn_off[i]), int(nn_off[i + 1])
            assert int(res[i]["n_query"]) == len(c["query"]) and int(res[i]["status"]) == (GOLDEN[name]["status"] & 3), name
            ratios = ac.compare(name, as_got(out[i], res[i], idx[a:b]), GOLDEN[name])
            for k, v in ratios.items():
                if v > worst[k][0]:
                    worst[k] = (v, name)
            unmatched = idx[a:b] == ac.NO_MATCH
            assert np.isposinf(d2[a:b][unmatched]).all() and (d2[a:b][~unmatched] <= c["max_dist"] ** 2).all(), name
            alone = Call(g, [name])
            try:
                o1, r1, _, i1, d1 = alone.run()
            finally:
                alone.free()
            assert o1[0].tobytes() == out[i].tobytes() and r1[0].tobytes() == res[i].tobytes(), name   # the same bits whatever else the call holds
            assert np.array_equal(i1, idx[a:b]) and d1.tobytes() == d2[a:b].tobytes(), name
        for k, (qi, ri) in enumerate(ex, start=len(names)):          # the pairs across cases, against the numpy statement
            q, r = ac.CASES[names[qi]]["query"], ac.CASES[names[ri]]["ref"]
            want = cloudmetrics.align(q, r, many.max_dist, None, many.max_iter, many.eps[0], many.eps[1], many.thr)
            assert (int(out[k]["iters"]), int(out[k]["status"]), int(out[k]["n_matched_first"])) == (want["iters"], want["status"], want["n_matched_first"]), (qi, ri)
            a, b = int(nn_off[k]), int(nn_off[k + 1])
            assert np.array_equal(idx[a:b], want["c2c"]["j"]) and int(res[k]["n_matched"]) == want["c2c"]["n_matched"], (qi, ri)
            T = np.r_[out[k]["rot"], out[k]["trans"]]
            assert np.abs(T[:9] - want["T"][:9]).max() <= 2 * ac.C_R * ac.ULP and np.abs(T[9:] - want["T"][9:]).max() <= 2 * ac.C_T * ac.ULP * 2.5, (qi, ri)
    print(f"\ndevice: worst ratios {worst} (C {ac.C_R}, {ac.C_T}, {ac.C_FIG})")


def test_far_case_agrees_with_the_same_case_at_the_origin(g):
    a, b = Call(g, ["far_origin"]), Call(g, ["far"])
    try:
        oa, ra, _, ia, _ = a.run()
        ob, rb, _, ib, _ = b.run()
    finally:
        a.free(), b.free()
    o = np.array([3000.0, 2000.0, 100.0])
    assert (int(oa[0]["iters"]), int(oa[0]["status"])) == (int(ob[0]["iters"]), int(ob[0]["status"])) and np.array_equal(ia, ib)
    Ra = oa[0]["rot"].reshape(3, 3)
    assert np.abs(oa[0]["rot"] - ob[0]["rot"]).max() <= 2 * ac.C_R * ac.ULP
    assert np.abs(ob[0]["trans"] - (oa[0]["trans"] + o - Ra @ o)).max() <= 2 * ac.C_T * ac.ULP * 3000.0 + 3 * 3000.0 * 2 * ac.C_R * ac.ULP
    assert abs(float(ra[0]["rmse"]) - float(rb[0]["rmse"])) <= 2 * ac.C_FIG * ac.ULP * ac.M


def test_optional_outputs_host_entry_and_poisoned_pools(g, hip_lib, clean_env):
    names = ac.groups()[MAIN]
    ex = extras(names)
    full, bare = Call(g, names, ex), Call(g, names, ex, with_nn=False)
    try:
        out, res, nn_off, idx, d2 = full.run()
        o0, r0, off0, _, _ = bare.run()
        assert o0.tobytes() == out.tobytes() and r0.tobytes() == res.tobytes() and np.array_equal(off0, nn_off)    # NULL nn outputs: the same records
        o1, r1, _, i1, d1 = full.run(want_c2c=False)
        assert r1 is None and o1.tobytes() == out.tobytes() and np.array_equal(i1, idx) and d1.tobytes() == d2.tobytes()   # NULL c2c_out
        o2, r2, _, _, _ = bare.run(want_c2c=False)
        assert r2 is None and o2.tobytes() == out.tobytes()
        ho, hr, hoff, hidx, hd2 = g.clouds_align(full.q, full.qo, full.r, full.ro, full.pairs, full.max_dist, full.T0, full.max_iter, full.eps[0], full.eps[1], full.thr,
                                                 want_nn=True)
        assert ho.tobytes() == out.tobytes() and hr.tobytes() == res.tobytes() and np.array_equal(hoff, nn_off) and np.array_equal(hidx, idx) and hd2.tobytes() == d2.tobytes()
        ho2, hr2, _ = g.clouds_align(full.q, full.qo, full.r, full.ro, full.pairs, full.max_dist, full.T0, full.max_iter, full.eps[0], full.eps[1], full.thr)
        assert ho2.tobytes() == out.tobytes() and hr2.tobytes() == res.tobytes()
    finally:
        full.free(), bare.free()
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        for with_nn in (True, False):
            p = Call(gp, names, ex, with_nn=with_nn)
            try:
                po, pr, _, pidx, pd2 = p.run()
            finally:
                p.free()
            assert po.tobytes() == out.tobytes() and pr.tobytes() == res.tobytes()
            if with_nn:
                assert np.array_equal(pidx, idx) and pd2.tobytes() == d2.tobytes()
        ho, hr, _ = gp.clouds_align(full.q, full.qo, full.r, full.ro, full.pairs, full.max_dist, full.T0, full.max_iter, full.eps[0], full.eps[1], full.thr)
        assert ho.tobytes() == out.tobytes() and hr.tobytes() == res.tobytes()
    finally:
        gp.close()


def test_status_pairs_leave_their_neighbours_alone(g):
    names = ac.groups()[MAIN]
    bad = ["nan_query", "nan_ref", "range_query", "bad_t0"]
    assert all(n in names for n in bad)
    a, b = Call(g, names), Call(g, [n for n in names if n not in bad])
    try:
        oa, ra, offa, ia, da = a.run()
        ob, rb, _, ib, _ = b.run()
    finally:
        a.free(), b.free()
    keep = [i for i, n in enumerate(names) if n not in bad]
    assert oa[keep].tobytes() == ob.tobytes() and ra[keep].tobytes() == rb.tobytes()
    assert np.array_equal(np.concatenate([ia[int(offa[i]):int(offa[i + 1])] for i in keep]), ib)
    for i, n in enumerate(names):
        if n in bad:
            r, c = oa[i], ac.CASES[n]
            assert int(r["status"]) == GOLDEN[n]["status"] and np.r_[r["rot"], r["trans"]].tobytes() == c["T0"].tobytes(), n
            assert (int(r["iters"]), int(r["n_matched_first"])) == (0, 0) and all(np.isnan(r[f]) for f in ("rmse_first", "step_rot", "step_trans")), n
            assert (ia[int(offa[i]):int(offa[i + 1])] == ac.NO_MATCH).all() and np.isposinf(da[int(offa[i]):int(offa[i + 1])]).all(), n
            assert int(ra[i]["n_matched"]) == 0 and np.isnan(ra[i]["rmse"]) and int(ra[i]["n_query"]) == 20, n


def raw_call(g, fn, query, n_q, q_off, ref, n_r, r_off, n_pairs, pq, pr, max_dist, thr, n_thr, T0, max_iter, eps_rot, eps_trans, out, c2c, idx, d2, nn_off):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = fn(g.h, ptr(query), C.c_size_t(n_q), arr(q_off), ptr(ref), C.c_size_t(n_r), arr(r_off), C.c_size_t(n_pairs), arr(pq), arr(pr), C.c_double(max_dist),
             arr(thr), C.c_uint32(n_thr), arr(T0), C.c_uint32(max_iter), C.c_double(eps_rot), C.c_double(eps_trans), arr(out), arr(c2c), ptr(idx), ptr(d2), arr(nn_off))
    return rc_, g.L.lk_last_error(g.h).decode()


def test_refusals(g):
    names = ["s3_65", "s63_64", "t0_answer"]
    call = Call(g, names, [(0, 1)])
    good, good_c, good_off, good_idx, good_d2 = call.run()
    n = len(call.pairs)
    Q, R_, I, D = call.gq.ptr, call.gr.ptr, call.gi.ptr, call.gd.ptr
    pq, pr = np.ascontiguousarray(call.pairs[:, 0]), np.ascontiguousarray(call.pairs[:, 1])
    thr = np.asarray(ac.THR, dtype=np.float64)
    T0 = np.ascontiguousarray(call.T0)
    base = dict(query=Q, n_q=len(call.qo) - 1, q_off=call.qo, ref=R_, n_r=len(call.ro) - 1, r_off=call.ro, n_pairs=n, pq=pq, pr=pr, max_dist=ac.M, thr=thr, n_thr=3,
                T0=T0, max_iter=ac.MAX_ITER, eps_rot=ac.EPS_ROT, eps_trans=ac.EPS_TRANS, idx=I, d2=D)
    dec_q, dec_r = call.qo.copy(), call.ro.copy()
    dec_q[1], dec_r[2] = dec_q[2] + 1, dec_r[1] - 1
    past_q, past_r = pq.copy(), pr.copy()
    past_q[1], past_r[2] = len(call.qo) - 1, 77
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                           # noqa: E731
    thr_of = lambda *v: np.array(v, dtype=np.float64)                                       # noqa: E731
    q_rec0 = Q + 16 * int(call.qo[0])
    refusals = [
        # every refusal of lk_clouds_c2c_dev
        (dict(n_pairs=0), -1, "n_pairs"), (dict(query=None), -1, "null argument (query)"), (dict(ref=None), -1, "null argument (ref)"),
        (dict(q_off=None), -1, "null argument (q_off)"), (dict(r_off=None), -1, "null argument (r_off)"), (dict(pq=None), -1, "null argument (pair_q)"),
        (dict(pr=None), -1, "null argument (pair_r)"),
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
        # and its own
        (dict(out=None), -1, "null argument (out)"), (dict(max_iter=1001), -1, "max_iter is 1001"), (dict(max_iter=0xFFFFFFFF), -1, "max_iter"),
        (dict(eps_rot=-1e-9), -1, "eps_rot"), (dict(eps_rot=np.nan), -1, "eps_rot"), (dict(eps_rot=np.inf), -1, "eps_rot"),
        (dict(eps_trans=-1.0), -1, "eps_trans"), (dict(eps_trans=np.nan), -1, "eps_trans"), (dict(eps_trans=-np.inf), -1, "eps_trans"),
    ]
    fresh = lambda dt, k: np.full(k, 0xFF, dtype=np.uint8).repeat(dt.itemsize).view(dt)      # noqa: E731
    try:
        for change, code, word in refusals:
            out, c2c = fresh(REC, n + 2), fresh(C2C, n + 2)
            nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(base, out=out, c2c=c2c, nn_off=nn_off)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_align_dev, **kw)
            assert rc_ == code and word in msg and "lk_clouds_align_dev: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)) and devguard.untouched(c2c.view(np.uint8)) and devguard.untouched(nn_off.view(np.uint8)), change
            call.gq.check(), call.gr.check()
            assert call.gi.check().tobytes() == good_idx.tobytes() and call.gd.check().tobytes() == good_d2.tobytes(), change
        again = call.run()                                                           # the handle is usable, a good call is right
        assert again[0].tobytes() == good.tobytes() and again[1].tobytes() == good_c.tobytes() and again[4].tobytes() == good_d2.tobytes()
        # the host entry refuses the same way, under its own name (4-byte alignment for its clouds)
        hq, hr = np.ascontiguousarray(call.q), np.ascontiguousarray(call.r)
        hi, hd = np.zeros(call.total, dtype=np.uint32), np.zeros(call.total, dtype=np.float64)
        hbase = dict(base, query=hq.ctypes.data, ref=hr.ctypes.data, idx=hi.ctypes.data, d2=hd.ctypes.data)
        for change, code, word in ((dict(n_pairs=0), -1, "n_pairs"), (dict(max_iter=1001), -1, "max_iter"), (dict(eps_trans=np.nan), -1, "eps_trans"),
                                   (dict(query=hq.ctypes.data + 2), -1, "query must be 4-byte aligned"), (dict(out=None), -1, "null argument (out)"),
                                   (dict(r_off=u64(0, 1, 2, 3, 1 << 31), n_r=4), -3, "2^31")):
            out, c2c = fresh(REC, n + 2), fresh(C2C, n + 2)
            nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(hbase, out=out, c2c=c2c, nn_off=nn_off)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_align, **kw)
            assert rc_ == code and word in msg and "lk_clouds_align: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)) and devguard.untouched(c2c.view(np.uint8)) and devguard.untouched(nn_off.view(np.uint8)), change
            assert not hi.any() and not hd.any(), change
        # a good call writes every byte of its n_pairs records and nothing behind them; T0 NULL is the identity; max_iter 1000 and eps 0 are accepted
        out, c2c = fresh(REC, n + 2), fresh(C2C, n + 2)
        nn_off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        rc_, msg = raw_call(g, g.L.lk_clouds_align_dev, **dict(base, out=out, c2c=c2c, nn_off=nn_off, idx=None, d2=None))
        assert rc_ == 0 and out[:n].tobytes() == good.tobytes() and c2c[:n].tobytes() == good_c.tobytes() and np.array_equal(nn_off, good_off), msg
        assert devguard.untouched(out[n:].view(np.uint8)) and devguard.untouched(c2c[n:].view(np.uint8))
        rc_, msg = raw_call(g, g.L.lk_clouds_align_dev, **dict(base, out=out, c2c=None, nn_off=None, idx=None, d2=None, thr=None, n_thr=0, T0=None, max_iter=1000,
                                                                eps_rot=0.0, eps_trans=0.0))
        # (the three cases converge from the identity by repeating a solve to the bit; the pair across cases matches fewer than three points)
        assert rc_ == 0 and out[:n]["status"].tolist() == [ac.CONVERGED] * 3 + [ac.FEW] and out[:n]["iters"].tolist()[3] == 0, msg
        assert (out[:3]["iters"] >= 2).all() and (out[:3]["iters"] < 10).all() and not out[:3]["step_rot"].any() and not out[:3]["step_trans"].any()
    finally:
        call.free()


# ---- lk_clouds_transform_dev

def transform_inputs():
    rng = np.random.default_rng(77)
    clouds = [rng.uniform(-40.0, 40.0, (n, 3)) for n in (0, 1, 63, 257, 0, 300)]
    rec, off = tcg.side(clouds)
    rec[:, 3].view(np.uint32)[:] = rng.integers(0, 2 ** 32, len(rec), dtype=np.uint32)       # w: any bits, NaN payloads among them
    rec.view(np.uint32)[5, 3] = 0x7FC12345
    rec[int(off[3]) + 1, :3] = [np.nan, np.inf, 1.0]                                         # non-finite coordinates go through as the arithmetic has them
    T = np.stack([ac.about(ac.rot(k % 3, 10.0 + 7.0 * k) @ ac.rot((k + 1) % 3, -33.0), np.array([1.0 + k, -2.0, 0.25 * k]), np.zeros(3)) for k in range(len(off) - 1)])
    T[2, 2] = 1e37                                                                           # a shear that overflows float32: +-inf, as numpy rounds it
    return rec, off, T


def expected_transform(rec, off, T):
    return np.concatenate([cloudmetrics.transform(rec[int(off[c]):int(off[c + 1])], T[c]) for c in range(len(off) - 1)])


def same_records(got, want):
    """Bit-equal records: every w, and every coordinate but for which NaN a NaN is (a NaN coordinate that the arithmetic made has no defined payload)."""
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    nan = np.isnan(want[:, :3])
    return (got.shape == want.shape and got[:, 3].tobytes() == want[:, 3].tobytes() and np.array_equal(np.isnan(got[:, :3]), nan)
            and got[:, :3][~nan].tobytes() == want[:, :3][~nan].tobytes())


def test_transform_out_of_place_and_in_place(g):
    rec, off, T = transform_inputs()
    want = expected_transform(rec, off, T)
    n = int(off[-1] - off[0])
    gin = devguard.Guarded.input(g, rec, offset=16, name="transform in")
    gout = devguard.Guarded(g, 16 * n, offset=16, name="transform out")
    try:
        g.clouds_transform_dev(gin.ptr, off, T, gout.ptr)
        gin.check()
        got = gout.read(np.float32).reshape(-1, 4)
        assert same_records(got, want) and np.isinf(want[:, :3]).any() and np.isnan(want[:, :3]).any()   # bit-equal to cloudmetrics.transform, w (NaN payloads) included
        assert got[:, 3].tobytes() == rec[int(off[0]):int(off[-1]), 3].tobytes()
        # in place: d_out = d_in + 4 * off[0] floats; the records in front of off[0] and the bands stay as they were
        g.clouds_transform_dev(gin.ptr, off, T, gin.ptr + 16 * int(off[0]))
        img = np.frombuffer(read_payload(g, gin), dtype=np.float32).reshape(-1, 4)
        assert same_records(img[int(off[0]):int(off[-1])], want) and img[:int(off[0])].tobytes() == rec[:int(off[0])].tobytes()
        assert img[int(off[-1]):].tobytes() == rec[int(off[-1]):].tobytes()
    finally:
        gin.free(), gout.free()


def read_payload(g, guarded):
    """The payload of a guarded INPUT that a call was allowed to rewrite, its bands verified."""
    lay = guarded.lay
    raw = np.zeros(lay.total, dtype=np.uint8)
    g.synchronize()
    g.d2h(raw, guarded.base)
    assert raw[:lay.lo].tobytes() == lay.pattern[:lay.lo].tobytes() and raw[lay.hi:].tobytes() == lay.pattern[lay.hi:].tobytes(), "a guard band of the in-place buffer was written"
    return raw[lay.lo:lay.hi].tobytes()


def test_transform_refusals(g):
    rec, off, T = transform_inputs()
    n = int(off[-1] - off[0])
    gin = devguard.Guarded.input(g, rec, offset=16, name="transform refusals in")
    gout = devguard.Guarded(g, 16 * n, offset=16, name="transform refusals out")
    fn = g.L.lk_clouds_transform_dev
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    nc = len(off) - 1
    dec = off.copy()
    dec[2] = dec[3] + 1
    badT = T.copy()
    badT[3, 10] = np.nan
    infT = T.copy()
    infT[0, 0] = np.inf
    first = gin.ptr + 16 * int(off[0])
    base = dict(d_in=gin.ptr, n=nc, off=off, T=T, d_out=gout.ptr)
    try:
        for change, code, word in [(dict(n=0), -1, "n_clouds is 0"), (dict(d_in=None), -1, "null argument (d_in)"), (dict(off=None), -1, "null argument (off)"),
                                   (dict(T=None), -1, "null argument (T)"), (dict(d_out=None), -1, "null argument (d_out)"),
                                   (dict(d_in=gin.ptr + 4), -1, "d_in must be 16-byte aligned"), (dict(d_out=gout.ptr + 8), -1, "d_out must be 16-byte aligned"),
                                   (dict(off=dec), -1, "off decreases at cloud 2"), (dict(T=badT), -1, "T[3]"), (dict(T=infT), -1, "T[0]"),
                                   (dict(d_out=first + 16), -1, "d_out overlaps d_in"), (dict(d_out=first - 16), -1, "d_out overlaps d_in"),
                                   (dict(d_out=gin.ptr), -1, "d_out overlaps d_in"),
                                   (dict(off=np.array([0, 1 << 32], dtype=np.uint64), n=1, T=T[:1].copy()), -3, "2^32 records")]:
            kw = dict(base)
            kw.update(change)
            rc_ = fn(g.h, ptr(kw["d_in"]), C.c_size_t(kw["n"]), arr(kw["off"]), arr(kw["T"]), ptr(kw["d_out"]))
            msg = g.L.lk_last_error(g.h).decode()
            assert rc_ == code and word in msg and "lk_clouds_transform_dev: " in msg, (change, rc_, msg)
            gin.check()
            devguard.untouched(gout.check())
        g.clouds_transform_dev(gin.ptr, off, T, gout.ptr)                                    # the handle is usable
        assert same_records(gout.read(np.float32), expected_transform(rec, off, T))
    finally:
        gin.free(), gout.free()


def test_c2c_on_the_transformed_cloud_agrees_with_the_final_search(g):
    """The tie to C2C, on every case whose generator asserts (c2c_tie) that no final distance lies within 4 * 2^-24 * L of the reach and no runner-up
    within that of the best: lk_clouds_c2c_dev on the float32 moved cloud matches the same points to the same neighbours, and its rmse is within
    4 * 2^-24 * L of the final search's - each coordinate moves by at most half a float32 ulp of L, a distance by at most sqrt(3) / 2 of one."""
    names = [n for n in ac.groups()[MAIN] if GOLDEN[n]["c2c_tie"] and ac.CASES[n]["kind"] == "posed"]
    assert len(names) >= 10 and "far" in names and "partial" in names
    call = Call(g, names)
    moved = devguard.Guarded(g, 16 * (int(call.qo[-1]) - int(call.qo[0])), offset=16, name="tie moved")
    gi, gd = devguard.Guarded(g, 4 * call.total, offset=4, name="tie idx"), devguard.Guarded(g, 8 * call.total, offset=8, name="tie d2")
    try:
        out, res, nn_off, idx, _ = call.run()
        T = np.concatenate([np.c_[out["rot"], out["trans"]], [ac.IDENTITY]])                 # (the trailing NaN cloud that no pair names)
        g.clouds_transform_dev(call.gq.ptr, call.qo, T, moved.ptr)
        rel = call.qo - call.qo[0]
        r2, off2 = g.clouds_c2c_dev(moved.ptr, rel, call.gr.ptr, call.ro, call.pairs, call.max_dist, call.thr, gi.ptr, gd.ptr)
        idx2 = gi.read(np.uint32)
        assert np.array_equal(off2, nn_off)
        for i, n in enumerate(names):
            a, b = int(nn_off[i]), int(nn_off[i + 1])
            assert int(r2[i]["n_matched"]) == int(res[i]["n_matched"]) == GOLDEN[n]["n_matched"] and np.array_equal(idx2[a:b], idx[a:b]), n
            assert abs(float(r2[i]["rmse"]) - float(res[i]["rmse"])) <= 4 * 2.0 ** -24 * ac.extent(ac.CASES[n]), n
    finally:
        call.free(), moved.free(), gi.free(), gd.free()


# ---- end to end: two runs replayed on the frozen map, their registered clouds downsampled, one moved by a known T and aligned back

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
    gw = devguard.Guarded(g, 16 * n, offset=16, name="align replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="align replay d_out")
    gm = devguard.Guarded(g, 16 * n, offset=16, name="align replay moved")
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * 2))
        _, sbo = g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, tmc.LEAF, go.ptr)
        m = int(out_off[-1])
        assert not unf.any() and m > 100
        img = go.check().copy()
        clouds = np.frombuffer(img[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        centre = clouds[:int(out_off[1]), :3].astype(np.float64).mean(0)
        known = np.stack([ac.about(ac.rot(2, 0.8) @ ac.rot(0, -0.5), np.array([0.02, -0.015, 0.01]), centre), ac.IDENTITY])
        B = int(sbo[-1])
        before = (g.batch_get_states(0, 2), trr.times_of(g, 2), g.runs_bucket_poses(0, B).tobytes(), g.map_export().copy())
        g.clouds_transform_dev(go.ptr, out_off, known, gm.ptr)                                # cloud 0 moved by a known T, cloud 1 as it is
        moved = np.frombuffer(gm.check()[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        assert same_records(moved, expected_transform(clouds, out_off, known))
        out, res, _ = g.clouds_align_dev(gm.ptr, out_off, go.ptr, out_off, [(0, 0), (1, 1)], 0.25, None, 30, 1e-7, 1e-9, (0.05, 0.1))
        assert go.check().tobytes() == img.tobytes(), "the call changed the map clouds"
        a_len = int(out_off[1])
        for k, (lo, hi) in enumerate(((0, a_len), (a_len, m))):
            want = cloudmetrics.align(moved[lo:hi], clouds[lo:hi], 0.25, None, 30, 1e-7, 1e-9, (0.05, 0.1))
            L = float(np.abs(clouds[lo:hi, :3]).max())
            T = np.r_[out[k]["rot"], out[k]["trans"]]
            assert (int(out[k]["iters"]), int(out[k]["status"]), int(out[k]["n_matched_first"])) == (want["iters"], want["status"], want["n_matched_first"]), k
            assert int(out[k]["status"]) == abi.LK_ALIGN_CONVERGED and int(res[k]["n_matched"]) == want["c2c"]["n_matched"] == hi - lo, k
            assert np.abs(T[:9] - want["T"][:9]).max() <= 2 * ac.C_R * ac.ULP and np.abs(T[9:] - want["T"][9:]).max() <= 2 * ac.C_T * ac.ULP * L, k   # (either side within tol of the truth)
            assert abs(float(res[k]["rmse"]) - want["c2c"]["rmse"]) <= 2 * ac.C_FIG * ac.ULP * 0.25, k
        # aligned back: T undoes the known motion up to the float32 rounding of the moved cloud
        back = np.r_[out[0]["rot"], out[0]["trans"]]
        Rk, tk = known[0][:9].reshape(3, 3), known[0][9:]
        assert np.abs(back[:9].reshape(3, 3) @ Rk - np.eye(3)).max() < 1e-6 and np.abs(back[:9].reshape(3, 3) @ tk + back[9:]).max() < 1e-4
        assert float(res[0]["rmse"]) < 1e-5 < float(out[0]["rmse_first"]) and int(out[1]["iters"]) == 1 and float(res[1]["rmse"]) == 0.0
        print(f"replay: map cloud of {a_len} points moved and aligned back in {int(out[0]['iters'])} solves, rmse {float(out[0]['rmse_first']):.4f} -> {float(res[0]['rmse']):.2e} m")
        after = (g.batch_get_states(0, 2), trr.times_of(g, 2), g.runs_bucket_poses(0, B).tobytes(), g.map_export())
        assert np.array_equal(after[0][0], before[0][0]) and np.array_equal(after[0][1], before[0][1]) and after[1] == before[1]
        assert after[2] == before[2] and np.array_equal(after[3], before[3])
    finally:
        g.device_free(d_pts)
        gw.free(), go.free(), gm.free()
        g.close()
