"""-m gpu: lk_clouds_sor_dev / lk_clouds_sor - outliers removed from many map clouds, on the device.

The cases are the frozen table of tests/sorcases.py, the expected values its exact / 50-digit evaluation (tests/golden/sor_cases.npz): keep, cnt, the
counts, worst, status, the output offsets, the output records and src_idx are compared exactly, dbar / mu / sigma / thr within the bounds derived
there.

Every call's clouds lie between the guard bands of tests/devguard.py at payload offset 16, behind three leading records of NaN that belong to nobody
(off[0] != 0); a cloud of NaN records sits in the middle of every call of several clouds; every record's w is a NaN with a payload of its own, so a
copy that is not bit for bit shows.  The outputs are guarded buffers of exactly off[n_clouds] - off[0] entries, so a write behind them lands in a
band, and what lies behind the kept records must still hold its fill."""
import ctypes as C
import itertools

import numpy as np
import pytest

import devguard
import scenes
import sorcases as sc
import test_map_clouds as tmc
import test_overlay_runs as tor
import test_replay_runs as trr
from legkilo_amd import abi, cloudmetrics

pytestmark = pytest.mark.gpu

GOLDEN = sc.golden()
REC = abi.sor_dtype()
LEAD = 3
NAN_CLOUD = np.full((5, 3), np.nan, dtype=np.float32)
OUTPUTS = (("out", 16, np.uint8), ("src", 4, np.uint32), ("keep", 1, np.uint8), ("cnt", 4, np.uint32), ("dbar", 8, np.float64))
MAIN = (sc.K, sc.REACH, sc.N_SIGMA)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("LEGKILO_POISON_POOLS", raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def g(hip_lib):
    h = tmc.new_handle(hip_lib)
    yield h
    h.close()


def records(clouds, lead=LEAD):
    """Clouds [n_i, 3] as one buffer of x y z w records behind `lead` records of NaN; w = a quiet NaN whose payload is the record's number ->
    (float32 [N, 4], offsets uint64 [len(clouds) + 1])."""
    parts = [np.full((lead, 3), np.nan, dtype=np.float32)] + [np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds]
    xyz = np.concatenate(parts)
    rec = np.zeros((len(xyz), 4), dtype=np.float32)
    rec[:, :3] = xyz
    rec.view(np.uint32)[:, 3] = 0x7FC00000 | (1 + np.arange(len(xyz), dtype=np.uint32))
    return rec, (lead + np.r_[0, np.cumsum([len(p) for p in parts[1:]])]).astype(np.uint64)


class Call:
    """Clouds as ONE call in guarded device memory; want = (out, src, keep, cnt, dbar): which outputs the call is given."""

    def __init__(self, g, clouds, k, reach, n_sigma, want=(True,) * 5, tag="sor"):
        self.g, self.k, self.reach, self.n_sigma = g, k, reach, n_sigma
        self.rec, self.off = records(clouds)
        self.total = int(self.off[-1] - self.off[0])
        tag = f"{tag} {len(clouds)} {self.total}"
        self.gc = devguard.Guarded.input(g, self.rec, offset=16, name=tag + " clouds")
        self.buf = [devguard.Guarded(g, size * self.total, offset=size, name=f"{tag} {name}") if w else None for (name, size, _), w in zip(OUTPUTS, want)]

    def run(self):
        """-> dict(res, off (or None), out uint32 [n_kept, 4], src, keep, cnt, dbar), None for an output not asked for; bands untouched, the input
        unmodified, every entry of the documented extent written and nothing behind it."""
        res, off = self.g.clouds_sor_dev(self.gc.ptr, self.off, self.k, self.reach, self.n_sigma, *[b.ptr if b else 0 for b in self.buf])
        self.gc.check()
        assert len(res) == len(self.off) - 1
        got = dict(res=res, off=off)
        for (name, size, dt), b in zip(OUTPUTS, self.buf):
            got[name] = None
            if b is None:
                continue
            raw = b.check()
            n = self.total if name not in ("out", "src") else int(off[-1])
            assert devguard.untouched(raw[size * n:]), name                  # nothing behind the kept records
            got[name] = np.frombuffer(raw[:size * n].tobytes(), dtype=np.uint32).reshape(n, 4) if name == "out" else np.frombuffer(raw[:size * n].tobytes(), dtype=dt)
            assert not n or devguard.sentinel_free(got[name]), name
        if off is not None:
            assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), res["n_kept"].astype(np.int64))
        return got

    def span(self, k):
        return int(self.off[k] - self.off[0]), int(self.off[k + 1] - self.off[0])

    def cloud_bits(self, k):
        """cloud k's input records as uint32 [n, 4]"""
        return self.rec[int(self.off[k]):int(self.off[k + 1])].view(np.uint32)

    def free(self):
        for b in [self.gc] + self.buf:
            if b:
                b.free()


def run_once(g, clouds, k, reach, n_sigma, want=(True,) * 5, tag="sor"):
    c = Call(g, clouds, k, reach, n_sigma, want, tag)
    try:
        return c, c.run()
    finally:
        c.free()


def with_nan_in_the_middle(names):
    """-> (clouds, index of each name's cloud)"""
    clouds = [sc.CASES[n]["cloud"] for n in names]
    if len(names) < 2:
        return clouds, list(range(len(names)))
    mid = len(names) // 2
    return clouds[:mid] + [NAN_CLOUD] + clouds[mid:], [i if i < mid else i + 1 for i in range(len(names))]


def cut(call, got, k):
    """cloud k's part of a call's results: (record, out, src, keep, cnt, dbar)"""
    a, b = call.span(k)
    lo, hi = int(got["off"][k]), int(got["off"][k + 1])
    return got["res"][k], got["out"][lo:hi], got["src"][lo:hi], got["keep"][a:b], got["cnt"][a:b], got["dbar"][a:b]


def check_case(name, bits, part, ratios, same_bits):
    """Decisions exactly, figures within tolerance; ratios: [worst dbar / mu ratio, worst sigma / thr ratio] against the bounds at C = 1, updated;
    same_bits: [dbar entries, of them equal to the numpy statement's to the bit], updated."""
    rec, out, src, keep, cnt, dbar = part
    c, want = sc.CASES[name], GOLDEN[name]
    assert int(rec["status"]) == want["status"] and int(rec["n_points"]) == len(c["cloud"]), name
    assert tuple(int(rec[f]) for f in ("n_isolated", "n_outliers", "n_kept", "worst")) == tuple(want[f] for f in ("n_isolated", "n_outliers", "n_kept", "worst")), name
    assert np.array_equal(keep, want["keep"]) and np.array_equal(cnt, want["cnt"]) and np.array_equal(np.isnan(dbar), np.isnan(want["dbar"])), name
    kept = np.flatnonzero(want["keep"])
    assert np.array_equal(src, kept) and np.array_equal(out, bits[kept]), name       # input order, all 16 bytes, w's payload included
    has = ~np.isnan(want["dbar"])
    for f in sc.FIGURES:
        assert np.isnan(rec[f]) == np.isnan(want[f]), (name, f)
    if not has.any():
        return
    td, ts = sc.tol_d(c, 1.0), sc.tol_s(c, want, 1.0)
    ed = max(np.abs(dbar[has] - want["dbar"][has]).max(), abs(float(rec["mu"]) - want["mu"])) / td
    ratios[0] = max(ratios[0], float(ed))
    assert ed <= sc.C_D, (name, ed)
    if want["sigma"] > 0.0:
        es = abs(float(rec["sigma"]) - want["sigma"]) / ts
        if not np.isinf(want["thr"]):
            es = max(es, abs(float(rec["thr"]) - want["thr"]) / ts)
        ratios[1] = max(ratios[1], float(es))
        assert es <= sc.C_S, (name, es)
    else:
        assert float(rec["sigma"]) == 0.0 and abs(float(rec["thr"]) - want["thr"]) <= sc.C_D * td, name
    if np.isinf(want["thr"]):
        assert float(rec["thr"]) == np.inf, name
    ref = cloudmetrics.sor(c["cloud"], c["k"], c["reach"], c["n_sigma"])
    same_bits[0] += int(has.sum())
    same_bits[1] += int((dbar[has].view(np.uint64) == ref["dbar"][has].view(np.uint64)).sum())
    same_bits[2] += int(all(np.float64(rec[f]).tobytes() == np.float64(ref[f]).tobytes() for f in sc.FIGURES))
    same_bits[3] += 1


def test_every_case_in_one_call_and_alone(g):
    ratios, same_bits = [0.0, 0.0], [0, 0, 0, 0]
    for (k, reach, n_sigma), names in sc.groups().items():
        clouds, at = with_nan_in_the_middle(names)
        many, got = run_once(g, clouds, k, reach, n_sigma)
        if len(names) > 1:
            mid = len(names) // 2
            rec, out, src, keep, cnt, dbar = cut(many, got, mid)
            assert int(rec["status"]) == abi.LK_SOR_NONFINITE and len(out) == 0 and not keep.any() and not cnt.any() and np.isnan(dbar).all()
        for name, i in zip(names, at):
            part = cut(many, got, i)
            check_case(name, many.cloud_bits(i), part, ratios, same_bits)
            alone, one = run_once(g, [sc.CASES[name]["cloud"]], k, reach, n_sigma)
            assert one["res"][0].tobytes() == part[0].tobytes(), name        # a cloud's record has the same bits whatever else the call holds
            assert np.array_equal(one["out"][:, :3], part[1][:, :3]) and np.array_equal(one["src"], part[2]) and np.array_equal(one["keep"], part[3]), name
            assert np.array_equal(one["cnt"], part[4]) and one["dbar"].tobytes() == part[5].tobytes(), name
    print(f"\ndevice: worst ratio dbar / mu {ratios[0]:.3f} (C_D {sc.C_D}), sigma / thr {ratios[1]:.3f} (C_S {sc.C_S}); dbar equal to the numpy statement's to the "
          f"bit in {same_bits[1]} of {same_bits[0]} entries, mu sigma thr in {same_bits[2]} of {same_bits[3]} clouds")


@pytest.fixture(scope="module")
def main_group():
    return sc.groups()[MAIN]


def same(a, b, want):
    assert a["res"].tobytes() == b["res"].tobytes(), want
    for name, _, _ in OUTPUTS:
        assert a[name] is None or a[name].tobytes() == b[name].tobytes(), (want, name)
    assert a["off"] is None or np.array_equal(a["off"], b["off"]), want


def test_null_outputs_host_entry_and_poisoned_pools(g, hip_lib, main_group, clean_env):
    clouds, _ = with_nan_in_the_middle(main_group)
    _, full = run_once(g, clouds, *MAIN)
    for want in itertools.product((False, True), repeat=5):            # every subset of the optional outputs NULL: the same bits
        if not all(want):
            same(run_once(g, clouds, *MAIN, want=want)[1], full, want)
    only_off = Call(g, clouds, *MAIN, want=(False,) * 5)                # the offsets alone
    try:
        res, off = g.clouds_sor_dev(only_off.gc.ptr, only_off.off, *MAIN, want_off=True)
        assert res.tobytes() == full["res"].tobytes() and np.array_equal(off, full["off"])
    finally:
        only_off.free()
    edge = [sc.CASES[n]["cloud"] for n in ("s1", "s0", "s257")]         # an empty cloud between one record and 257, the offsets alone
    _, edge_full = run_once(g, edge, *MAIN)
    edge_off = Call(g, edge, *MAIN, want=(False,) * 5)
    try:
        res, off = g.clouds_sor_dev(edge_off.gc.ptr, edge_off.off, *MAIN, want_off=True)
        assert res.tobytes() == edge_full["res"].tobytes() and np.array_equal(off, edge_full["off"]) and off[1] == off[2]
        assert np.array_equal(np.diff(off.astype(np.int64)), res["n_kept"].astype(np.int64)) and res["n_points"].tolist() == [1, 0, 257]
    finally:
        edge_off.free()
    rec, roff = records(clouds)
    hres, hout, hoff, hsrc, hkeep, hcnt, hdbar = g.clouds_sor(rec, roff, *MAIN, want_points=True)
    assert hres.tobytes() == full["res"].tobytes() and np.array_equal(hoff, full["off"]) and np.array_equal(hout.view(np.uint32), full["out"])
    assert np.array_equal(hsrc, full["src"]) and np.array_equal(hkeep, full["keep"]) and np.array_equal(hcnt, full["cnt"]) and hdbar.tobytes() == full["dbar"].tobytes()
    short = g.clouds_sor(rec, roff, *MAIN)
    assert short[0].tobytes() == full["res"].tobytes() and np.array_equal(short[1].view(np.uint32), full["out"]) and np.array_equal(short[3], full["src"])
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        for want in ((True,) * 5, (False,) * 5, (True, False, False, False, False), (False, False, True, False, False)):
            same(run_once(gp, clouds, *MAIN, want=want)[1], full, want)
        assert gp.clouds_sor(rec, roff, *MAIN)[0].tobytes() == full["res"].tobytes()
    finally:
        gp.close()


def test_status_clouds_leave_their_neighbours_alone(g, main_group):
    """The group's call with and without the two non-finite cases: every other cloud keeps its bits, and a status cloud comes out empty."""
    bad = ["nan_cloud", "inf_cloud"]
    assert all(b in main_group for b in bad)
    a, ga = run_once(g, [sc.CASES[n]["cloud"] for n in main_group], *MAIN)
    b, gb = run_once(g, [sc.CASES[n]["cloud"] for n in main_group if n not in bad], *MAIN)
    keep_i = [i for i, n in enumerate(main_group) if n not in bad]
    assert ga["res"][keep_i].tobytes() == gb["res"].tobytes()
    for j, i in enumerate(keep_i):
        pa, pb = cut(a, ga, i), cut(b, gb, j)
        assert np.array_equal(pa[1][:, :3], pb[1][:, :3]) and all(x.tobytes() == y.tobytes() for x, y in zip(pa[2:], pb[2:])), main_group[i]
    for i, name in enumerate(main_group):
        if name in bad:
            r, out, src, keep, cnt, dbar = cut(a, ga, i)
            assert int(r["status"]) == abi.LK_SOR_NONFINITE and all(np.isnan(r[f]) for f in sc.FIGURES) and int(r["n_points"]) == 60
            assert (int(r["n_isolated"]), int(r["n_outliers"]), int(r["n_kept"]), int(r["worst"])) == (0, 0, 0, 0)
            assert len(out) == 0 and len(src) == 0 and not keep.any() and not cnt.any() and np.isnan(dbar).all()
    names = ["range_at", "range_below"]                                          # out of range: its own group (reach 2^-10)
    c = sc.CASES["range_at"]
    call, got = run_once(g, [sc.CASES[n]["cloud"] for n in names], c["k"], c["reach"], c["n_sigma"])
    assert got["res"]["status"].tolist() == [abi.LK_SOR_RANGE, 0] and got["off"].tolist() == [0, 0, 4] and got["keep"].tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert got["cnt"].tolist() == [0, 0, 0] + GOLDEN["range_below"]["cnt"].tolist() and int(got["res"][0]["n_points"]) == 3


def raw_call(g, fn, clouds, n_clouds, off, k, reach, n_sigma, out, d_out, out_off, src, keep, cnt, dbar):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = fn(g.h, ptr(clouds), C.c_size_t(n_clouds), arr(off), C.c_uint32(k), C.c_double(reach), C.c_double(n_sigma), arr(out), ptr(d_out), arr(out_off), ptr(src),
             ptr(keep), ptr(cnt), ptr(dbar))
    return rc_, g.L.lk_last_error(g.h).decode()


def test_refusals(g):
    names = ["s65", "duplicates", "s6"]
    call = Call(g, [sc.CASES[n]["cloud"] for n in names], *MAIN)
    good = call.run()
    nc = len(names)
    P = call.gc.ptr
    O, S, K, N, D = (b.ptr for b in call.buf)
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                           # noqa: E731
    base = dict(clouds=P, n_clouds=nc, off=call.off, k=MAIN[0], reach=MAIN[1], n_sigma=MAIN[2], d_out=O, src=S, keep=K, cnt=N, dbar=D)
    dec = call.off.copy()
    dec[1] = dec[2] + 1
    rec0 = P + 16 * int(call.off[0])
    refusals = [
        (dict(n_clouds=0), -1, "n_clouds"), (dict(clouds=None), -1, "null argument (clouds)"), (dict(off=None), -1, "null argument (off)"),
        (dict(out=None), -1, "null argument (out)"), (dict(clouds=P + 8), -1, "clouds must be 16-byte aligned"), (dict(off=dec), -1, "off decreases at cloud 1"),
        (dict(k=0), -1, "k is 0"), (dict(k=33), -1, "k is 33"), (dict(reach=0.0), -1, "reach"), (dict(reach=-1.0), -1, "reach"), (dict(reach=np.nan), -1, "reach"),
        (dict(reach=np.inf), -1, "reach"), (dict(n_sigma=np.nan), -1, "n_sigma"), (dict(n_sigma=-0.5), -1, "n_sigma"), (dict(n_sigma=-np.inf), -1, "n_sigma"),
        (dict(out_off=None), -1, "out_cloud needs out_off"), (dict(out_off=None, d_out=None), -1, "src_idx needs out_off"),
        (dict(d_out=O + 8), -1, "out_cloud must be 16-byte aligned"), (dict(src=S + 2), -1, "src_idx must be 4-byte aligned"), (dict(cnt=N + 2), -1, "cnt must be 4-byte aligned"),
        (dict(dbar=D + 4), -1, "dbar must be 8-byte aligned"),
        (dict(d_out=rec0 + 16), -1, "out_cloud overlaps the input clouds"), (dict(src=rec0), -1, "src_idx overlaps the input clouds"),
        (dict(keep=P + 16 * int(call.off[-1]) - 1), -1, "keep overlaps the input clouds"), (dict(cnt=rec0 + 4), -1, "cnt overlaps the input clouds"),
        (dict(dbar=rec0 + 8), -1, "dbar overlaps the input clouds"), (dict(src=O + 16), -1, "out_cloud overlaps src_idx"), (dict(keep=S + 1), -1, "src_idx overlaps keep"),
        (dict(cnt=K + 3), -1, "keep overlaps cnt"), (dict(dbar=N + 4), -1, "cnt overlaps dbar"), (dict(dbar=O + 8), -1, "out_cloud overlaps dbar"),
        (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31 records or more"),
    ]
    try:
        for change, code, word in refusals:
            out = np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
            ooff = np.full(nc + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(base, out=out, out_off=ooff)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_sor_dev, **kw)
            assert rc_ == code and word in msg and "lk_clouds_sor_dev: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)) and devguard.untouched(ooff.view(np.uint8)), change   # a refused call writes nothing
            call.gc.check()
            for (name, size, _), b in zip(OUTPUTS, call.buf):
                n = call.total if name not in ("out", "src") else int(good["off"][-1])
                assert b.check()[:size * n].tobytes() == good[name].tobytes(), (change, name)
        again = call.run()                                                                  # the handle is usable, a good call is right
        same(again, good, "after the refusals")
        # the host entry refuses the same way, under its own name (4-byte alignment for its clouds)
        hc = np.ascontiguousarray(call.rec)
        T = call.total
        ho, hs, hk, hn, hd = np.zeros((T, 4), dtype=np.float32), np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.uint8), np.zeros(T, dtype=np.uint32), np.zeros(T)
        hbase = dict(base, clouds=hc.ctypes.data, d_out=ho.ctypes.data, src=hs.ctypes.data, keep=hk.ctypes.data, cnt=hn.ctypes.data, dbar=hd.ctypes.data)
        for change, code, word in ((dict(n_clouds=0), -1, "n_clouds"), (dict(reach=np.nan), -1, "reach"), (dict(clouds=hc.ctypes.data + 2), -1, "clouds must be 4-byte aligned"),
                                   (dict(k=0), -1, "k is 0"), (dict(n_sigma=-1.0), -1, "n_sigma"), (dict(out_off=None), -1, "out_off"),
                                   (dict(dbar=hc.ctypes.data + 16 * LEAD), -1, "dbar overlaps the input clouds"), (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31")):
            out = np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
            ooff = np.full(nc + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            kw = dict(hbase, out=out, out_off=ooff)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_sor, **kw)
            assert rc_ == code and word in msg and "lk_clouds_sor: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)) and devguard.untouched(ooff.view(np.uint8)), change
            assert not ho.any() and not hs.any() and not hk.any() and not hn.any() and not hd.any(), change
        # a good call writes every byte of its n_clouds records and n_clouds + 1 offsets and nothing behind them
        out = np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
        ooff = np.full(nc + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        rc_, msg = raw_call(g, g.L.lk_clouds_sor_dev, **dict(base, out=out, out_off=ooff, d_out=None, src=None, keep=None, cnt=None, dbar=None))
        assert rc_ == 0 and out[:nc].tobytes() == good["res"].tobytes() and devguard.untouched(out[nc:].view(np.uint8)), msg
        assert np.array_equal(ooff[:nc + 1], good["off"]) and devguard.untouched(ooff[nc + 1:].view(np.uint8))
    finally:
        call.free()


def test_cnt_plus_one_is_the_mme_count(g, main_group):
    """d_cnt + 1 == lk_clouds_mme_dev's d_n at the same radius, on the same clouds in the same buffer."""
    clouds, _ = with_nan_in_the_middle(main_group)
    call = Call(g, clouds, *MAIN, want=(False, False, False, True, False))
    gn = devguard.Guarded(g, 4 * call.total, offset=4, name="sor mme n")
    try:
        got = call.run()
        res = g.clouds_mme_dev(call.gc.ptr, call.off, sc.REACH, 5, gn.ptr)
        n = gn.read(np.uint32)
        ok = np.repeat(res["status"] == 0, np.diff(call.off.astype(np.int64)))
        assert ok.sum() > 1000 and np.array_equal(got["cnt"][ok] + 1, n[ok]) and not got["cnt"][~ok].any() and not n[~ok].any()
    finally:
        call.free(), gn.free()


def test_the_output_feeds_mme_and_c2c_and_src_idx_gathers_the_input(g):
    """d_out / out_off go into lk_clouds_mme_dev and lk_clouds_c2c_dev as they are, with the records cloudmetrics gives on the filtered clouds; the
    input gathered through d_src_idx is d_out."""
    names = ["strays", "s257", "s0", "k1"]
    clouds = [sc.CASES[n]["cloud"] for n in names]
    call = Call(g, clouds, *MAIN)
    try:
        got = call.run()
        off = got["off"]
        for i in range(len(names)):
            lo, hi = int(off[i]), int(off[i + 1])
            assert np.array_equal(call.cloud_bits(i)[got["src"][lo:hi]], got["out"][lo:hi]), names[i]
        assert int(got["res"][0]["n_kept"]) == 257 and int(got["res"][0]["n_isolated"]) == 4 and int(got["res"][0]["n_outliers"]) == 5
        filtered = [got["out"][int(off[i]):int(off[i + 1])].view(np.float32)[:, :3] for i in range(len(names))]
        d_out = call.buf[0].ptr
        mres = g.clouds_mme_dev(d_out, off, sc.REACH, 5)
        cres, _ = g.clouds_c2c_dev(d_out, off, call.gc.ptr, call.off, [(i, i) for i in range(len(names))], sc.REACH, thr=(0.05,))
        call.buf[0].check(), call.gc.check()
        for i, name in enumerate(names):
            wm = cloudmetrics.mme(filtered[i], sc.REACH, 5)
            assert (int(mres[i]["n_points"]), int(mres[i]["n_dense"]), int(mres[i]["n_scored"]), int(mres[i]["n_pairs"])) == (len(filtered[i]), wm["n_dense"], wm["n_scored"],
                                                                                                                            wm["n_pairs"]), name
            wc = cloudmetrics.c2c(filtered[i], clouds[i], sc.REACH, (0.05,))
            assert (int(cres[i]["n_query"]), int(cres[i]["n_matched"]), int(cres[i]["n_within"][0])) == (len(filtered[i]), wc["n_matched"], wc["n_within"][0]), name
            assert not len(filtered[i]) or float(cres[i]["max"]) == 0.0, name               # every kept record is a record of its input cloud
    finally:
        call.free()


# ---- end to end: a run replayed on the frozen map, its registered cloud downsampled, strays injected, the filter run where the cloud lies

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
    gw = devguard.Guarded(g, 16 * n, offset=16, name="sor replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="sor replay d_out")
    call = None
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * 2))
        g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, tmc.LEAF, go.ptr)
        assert not unf.any()
        a_len = int(out_off[1])
        cloud = np.frombuffer(go.check()[:16 * a_len].tobytes(), dtype=np.float32).reshape(a_len, 4)[:, :3]
        assert a_len > 5000
        # 40 strays beyond the cloud's corner, three reaches from the cloud and from each other, spread through the records
        k, reach, n_sigma = 8, 5.0 * tmc.LEAF, 2.0
        strays = (cloud.max(0).astype(np.float64) + 3.0 * reach * np.c_[1 + np.arange(40), np.ones(40), np.ones(40)]).astype(np.float32)
        at = np.linspace(0, a_len, 40, endpoint=False).astype(np.int64)
        mixed = np.insert(cloud, at, strays, axis=0)
        is_stray = np.zeros(len(mixed), dtype=bool)
        is_stray[at + np.arange(40)] = True
        assert np.array_equal(mixed[is_stray], strays)
        want = None
        for _ in range(8):                                                       # (n_sigma moves by 1e-3 until no point lies near the threshold)
            want = cloudmetrics.sor(mixed, k, reach, n_sigma)
            case = dict(reach=reach)
            tol = sc.tol_d(case) + sc.tol_s(case, want)
            near = np.abs(want["dbar"][~np.isnan(want["dbar"])] - want["thr"])
            if near.min() >= 1024 * tol:
                break
            n_sigma += 1e-3
        assert near.min() >= 1024 * tol, "no n_sigma leaves every dbar clear of the threshold"
        assert not want["keep"][is_stray].any() and (want["cnt"][is_stray] == 0).all() and want["n_isolated"] >= 40
        call = Call(g, [mixed], k, reach, n_sigma, tag="sor replay")
        got = call.run()
        r = got["res"][0]
        assert np.array_equal(got["keep"].astype(bool), want["keep"]) and np.array_equal(got["cnt"], want["cnt"])    # no point excused
        assert not got["keep"][is_stray].any() and np.array_equal(got["src"], want["src_idx"])
        assert np.array_equal(got["out"], call.cloud_bits(0)[want["keep"]])
        assert (int(r["status"]), int(r["n_points"]), int(r["n_isolated"]), int(r["n_outliers"]), int(r["n_kept"]), int(r["worst"])) == (
            0, len(mixed), want["n_isolated"], want["n_outliers"], want["n_kept"], want["worst"])
        has = ~np.isnan(want["dbar"])
        assert np.array_equal(np.isnan(got["dbar"]), ~has) and np.abs(got["dbar"][has] - want["dbar"][has]).max() <= 2 * sc.tol_d(case)   # either side within its bound of the truth
        assert abs(float(r["mu"]) - want["mu"]) <= 2 * sc.tol_d(case) and abs(float(r["sigma"]) - want["sigma"]) <= 2 * sc.tol_s(case, want)
        assert abs(float(r["thr"]) - want["thr"]) <= 2 * sc.tol_s(case, want)
        bits = int((got["dbar"][has].view(np.uint64) == want["dbar"][has].view(np.uint64)).sum())
        print(f"\nreplay: map cloud of {a_len} points + 40 strays at k = {k}, reach = {reach}, n_sigma = {n_sigma}: isolated {int(r['n_isolated'])}, outliers "
              f"{int(r['n_outliers'])}, kept {int(r['n_kept'])}, mu {float(r['mu']):.4f} sigma {float(r['sigma']):.4f} thr {float(r['thr']):.4f}; nearest dbar to thr "
              f"{near.min():.2e} m; dbar equal to numpy's to the bit in {bits} of {int(has.sum())}")
    finally:
        g.device_free(d_pts)
        gw.free(), go.free()
        if call:
            call.free()
        g.close()
