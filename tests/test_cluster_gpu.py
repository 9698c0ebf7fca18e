"""-m gpu: lk_clouds_cluster_dev / lk_clouds_cluster - many map clouds clustered (DBSCAN, connected components), on the device.

The cases are the frozen table of tests/clustercases.py, the expected values its exact evaluation (tests/golden/cluster_cases.npz): every value is a
whole number and is compared exactly - n, kind and label per point, size and first core index per cluster, the counts, the offsets, the output
records and src_idx.

Every call's clouds lie between the guard bands of tests/devguard.py at payload offset 16, behind three leading records of NaN that belong to nobody
(off[0] = 3); a cloud of NaN records sits in the middle of every call of several clouds; every record's w is a NaN with a payload of its own, so a
copy that is not bit for bit shows.  The outputs are guarded buffers of exactly off[n_clouds] - off[0] entries, so a write behind them lands in a
band, and what lies behind the clusters and the kept records must still hold its fill."""
import ctypes as C
import itertools

import numpy as np
import pytest

import clustercases as cc
import devguard
import scenes
import test_map_clouds as tmc
import test_overlay_runs as tor
import test_replay_runs as trr
import test_sor_gpu as tsg
from legkilo_amd import abi, cloudmetrics

pytestmark = pytest.mark.gpu

GOLDEN = cc.golden()
REC = abi.cluster_dtype()
LEAD = tsg.LEAD
NAN_CLOUD = tsg.NAN_CLOUD
records = tsg.records
OUTPUTS = (("label", 4, np.uint32), ("kind", 1, np.uint8), ("n", 4, np.uint32), ("cl_size", 4, np.uint32), ("cl_first", 4, np.uint32), ("out", 16, np.uint8),
           ("src", 4, np.uint32))
ALL = (True,) * len(OUTPUTS)
NONE = (False,) * len(OUTPUTS)
MAIN = cc.MAIN


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
    """Clouds as ONE call in guarded device memory; want: which of OUTPUTS the call is given."""

    def __init__(self, g, clouds, par, want=ALL, tag="cluster"):
        self.g, self.par = g, par
        self.rec, self.off = records(clouds)
        self.total = int(self.off[-1] - self.off[0])
        tag = f"{tag} {len(clouds)} {self.total}"
        self.gc = devguard.Guarded.input(g, self.rec, offset=16, name=tag + " clouds")
        self.buf = [devguard.Guarded(g, size * self.total, offset=size, name=f"{tag} {name}") if w else None for (name, size, _), w in zip(OUTPUTS, want)]

    def extent(self, name, got):
        return self.total if name in ("label", "kind", "n") else int(got["cl_off"][-1]) if name.startswith("cl_") else int(got["off"][-1])

    def run(self, want_cl_off=None, want_off=None):
        """-> dict(res, cl_off, off (or None), and per output its array or None); bands untouched, the input unmodified, every entry of the documented
        extent written and nothing behind it."""
        reach, min_pts, min_size, max_size, flags = self.par
        res, cl_off, off = self.g.clouds_cluster_dev(self.gc.ptr, self.off, reach, min_pts, min_size, max_size, flags, *[b.ptr if b else 0 for b in self.buf],
                                                     want_cl_off=want_cl_off, want_off=want_off)
        self.gc.check()
        assert len(res) == len(self.off) - 1
        got = dict(res=res, cl_off=cl_off, off=off)
        for (name, size, dt), b in zip(OUTPUTS, self.buf):
            got[name] = None
            if b is None:
                continue
            raw = b.check()
            n = self.extent(name, got)
            assert devguard.untouched(raw[size * n:]), name                  # nothing behind the documented extent
            got[name] = np.frombuffer(raw[:size * n].tobytes(), dtype=np.uint32).reshape(n, 4) if name == "out" else np.frombuffer(raw[:size * n].tobytes(), dtype=dt)
            assert not n or name == "label" or devguard.sentinel_free(got[name]), name   # (0xffffffff is the label of a noise point)
        if off is not None:
            assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), res["n_kept"].astype(np.int64))
        if cl_off is not None:
            assert cl_off[0] == 0 and np.array_equal(np.diff(cl_off.astype(np.int64)), res["n_clusters"].astype(np.int64))
        assert not res["pad"].any()
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


def run_once(g, clouds, par, want=ALL, tag="cluster", **kw):
    c = Call(g, clouds, par, want, tag)
    try:
        return c, c.run(**kw)
    finally:
        c.free()


def with_nan_in_the_middle(names):
    """-> (clouds, index of each name's cloud)"""
    clouds = [cc.CASES[n]["cloud"] for n in names]
    if len(names) < 2:
        return clouds, list(range(len(names)))
    mid = len(names) // 2
    return clouds[:mid] + [NAN_CLOUD] + clouds[mid:], [i if i < mid else i + 1 for i in range(len(names))]


def cut(call, got, k):
    """cloud k's part of a call's results: (record, label, kind, n, cl_size, cl_first, out, src)"""
    a, b = call.span(k)
    lo, hi = int(got["off"][k]), int(got["off"][k + 1])
    cl, ch = int(got["cl_off"][k]), int(got["cl_off"][k + 1])
    return got["res"][k], got["label"][a:b], got["kind"][a:b], got["n"][a:b], got["cl_size"][cl:ch], got["cl_first"][cl:ch], got["out"][lo:hi], got["src"][lo:hi]


def check_case(name, bits, part):
    """every value exactly"""
    rec, label, kind, n, cl_size, cl_first, out, src = part
    c, want = cc.CASES[name], GOLDEN[name]
    assert int(rec["n_points"]) == len(c["cloud"]) and all(int(rec[f]) == want[f] for f in cc.COUNTS), (name, rec, {f: want[f] for f in cc.COUNTS})
    assert np.array_equal(label, want["label"]) and np.array_equal(kind, want["kind"]) and np.array_equal(n, want["n"]), name
    assert np.array_equal(cl_size, want["cl_size"]) and np.array_equal(cl_first, want["cl_first"]), name
    kept = np.flatnonzero(want["keep"])
    assert np.array_equal(src, kept) and np.array_equal(out, bits[kept]), name       # input order, all 16 bytes, w's payload included
    assert want["status"] or int(rec["n_points"]) == int(rec["n_core"]) + int(rec["n_border"]) + int(rec["n_noise"]), name


def nan_part_is_empty(part):
    rec, label, kind, n, cl_size, cl_first, out, src = part
    assert int(rec["status"]) == abi.LK_CLUSTER_NONFINITE and int(rec["n_points"]) == len(label)
    assert not any(int(rec[f]) for f in cc.COUNTS if f != "status")
    assert (label == abi.LK_CLUSTER_NOISE).all() and not kind.any() and not n.any() and len(cl_size) == len(cl_first) == len(out) == len(src) == 0


def same(a, b, want):
    assert a["res"].tobytes() == b["res"].tobytes(), want
    for name, _, _ in OUTPUTS:
        assert a[name] is None or a[name].tobytes() == b[name].tobytes(), (want, name)
    for t in ("off", "cl_off"):
        assert a[t] is None or np.array_equal(a[t], b[t]), (want, t)


def test_every_case_in_one_call_and_alone_and_twice(g):
    for par, names in cc.groups().items():
        clouds, at = with_nan_in_the_middle(names)
        call = Call(g, clouds, par)
        try:
            got = call.run()
            same(call.run(), got, "the same call again")                 # identical bits in every output from run to run
        finally:
            call.free()
        if len(names) > 1:
            nan_part_is_empty(cut(call, got, len(names) // 2))
        for name, i in zip(names, at):
            part = cut(call, got, i)
            check_case(name, call.cloud_bits(i), part)
            _, one = run_once(g, [cc.CASES[name]["cloud"]], par)
            assert one["res"][0].tobytes() == part[0].tobytes(), name        # a cloud's record has the same bits whatever else the call holds
            for k, f in enumerate(("label", "kind", "n", "cl_size", "cl_first")):
                assert one[f].tobytes() == part[1 + k].tobytes(), (name, f)
            assert np.array_equal(one["out"][:, :3], part[6][:, :3]) and np.array_equal(one["src"], part[7]), name


@pytest.fixture(scope="module")
def main_group():
    return cc.groups()[MAIN]


def test_null_outputs_host_entry_and_poisoned_pools(g, hip_lib, main_group, clean_env):
    clouds, _ = with_nan_in_the_middle(main_group)
    _, full = run_once(g, clouds, MAIN)
    for want in itertools.product((False, True), repeat=len(OUTPUTS)):  # every subset of the optional outputs NULL: the same bits
        if not all(want):
            same(run_once(g, clouds, MAIN, want=want)[1], full, want)
    _, tables = run_once(g, clouds, MAIN, want=NONE, want_cl_off=True, want_off=True)     # the two offset tables alone
    assert tables["res"].tobytes() == full["res"].tobytes() and np.array_equal(tables["off"], full["off"]) and np.array_equal(tables["cl_off"], full["cl_off"])
    rec, roff = records(clouds)
    h = g.clouds_cluster(rec, roff, *MAIN)
    assert h["res"].tobytes() == full["res"].tobytes() and np.array_equal(h["out_off"], full["off"]) and np.array_equal(h["cl_off"], full["cl_off"])
    assert np.array_equal(h["out"].view(np.uint32), full["out"]) and np.array_equal(h["src_idx"], full["src"])
    for f in ("label", "kind", "n", "cl_size", "cl_first"):
        assert np.array_equal(h[f], full[f]), f
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        for want in (ALL, NONE, (True,) + (False,) * 6, (False,) * 5 + (True, False), (False, False, False, True, True, False, False)):
            same(run_once(gp, clouds, MAIN, want=want)[1], full, want)
        assert gp.clouds_cluster(rec, roff, *MAIN)["res"].tobytes() == full["res"].tobytes()
    finally:
        gp.close()


def test_status_clouds_leave_their_neighbours_alone(g, main_group):
    """The group's call with and without the two non-finite cases: every other cloud keeps its bits, and a status cloud comes out empty."""
    bad = ["nan_cloud", "inf_cloud"]
    assert all(b in main_group for b in bad)
    a, ga = run_once(g, [cc.CASES[n]["cloud"] for n in main_group], MAIN)
    b, gb = run_once(g, [cc.CASES[n]["cloud"] for n in main_group if n not in bad], MAIN)
    keep_i = [i for i, n in enumerate(main_group) if n not in bad]
    assert ga["res"][keep_i].tobytes() == gb["res"].tobytes()
    for j, i in enumerate(keep_i):
        pa, pb = cut(a, ga, i), cut(b, gb, j)
        assert np.array_equal(pa[6][:, :3], pb[6][:, :3]) and all(x.tobytes() == y.tobytes() for x, y in zip(pa[1:6] + pa[7:], pb[1:6] + pb[7:])), main_group[i]
    for i, name in enumerate(main_group):
        if name in bad:
            part = cut(a, ga, i)
            nan_part_is_empty(part)
            assert int(part[0]["n_points"]) == 60
    names = ["range_at", "range_below"]                                          # out of range: its own group (reach 2^-10)
    call, got = run_once(g, [cc.CASES[n]["cloud"] for n in names], cc.params(cc.CASES["range_at"]))
    assert got["res"]["status"].tolist() == [abi.LK_CLUSTER_RANGE, 0] and got["off"].tolist() == [0, 0, 4] and got["cl_off"].tolist() == [0, 0, 2]
    assert got["label"].tolist() == [abi.LK_CLUSTER_NOISE] * 3 + [0, 1, 0, 1] and got["n"].tolist() == [0, 0, 0, 2, 2, 2, 2] and int(got["res"][0]["n_points"]) == 3


def raw_call(g, fn, clouds, n_clouds, off, reach, min_pts, min_size, max_size, flags, out, label, kind, n, cl_size, cl_first, cl_off, d_out, out_off, src):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = fn(g.h, ptr(clouds), C.c_size_t(n_clouds), arr(off), C.c_double(reach), C.c_uint32(min_pts), C.c_uint32(min_size), C.c_uint32(max_size), C.c_uint32(flags),
             arr(out), ptr(label), ptr(kind), ptr(n), ptr(cl_size), ptr(cl_first), arr(cl_off), ptr(d_out), arr(out_off), ptr(src))
    return rc_, g.L.lk_last_error(g.h).decode()


def fresh_host_outputs(nc):
    return (np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC), np.full(nc + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64),
            np.full(nc + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))


def test_refusals(g):
    names = ["s65", "bridge", "s2"]
    call = Call(g, [cc.CASES[n]["cloud"] for n in names], MAIN)
    good = call.run()
    nc = len(names)
    P = call.gc.ptr
    L, K, N, CS, CF, O, S = (b.ptr for b in call.buf)
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                           # noqa: E731
    base = dict(clouds=P, n_clouds=nc, off=call.off, reach=MAIN[0], min_pts=MAIN[1], min_size=MAIN[2], max_size=MAIN[3], flags=MAIN[4], label=L, kind=K, n=N, cl_size=CS,
                cl_first=CF, d_out=O, src=S)
    dec = call.off.copy()
    dec[1] = dec[2] + 1
    rec0 = P + 16 * int(call.off[0])
    refusals = [
        (dict(n_clouds=0), -1, "n_clouds"), (dict(clouds=None), -1, "null argument (clouds)"), (dict(off=None), -1, "null argument (off)"),
        (dict(out=None), -1, "null argument (out)"), (dict(clouds=P + 8), -1, "clouds must be 16-byte aligned"), (dict(off=dec), -1, "off decreases at cloud 1"),
        (dict(reach=0.0), -1, "reach"), (dict(reach=-1.0), -1, "reach"), (dict(reach=np.nan), -1, "reach"), (dict(reach=np.inf), -1, "reach"),
        (dict(min_pts=0), -1, "min_pts is 0"), (dict(min_size=9, max_size=8), -1, "min_size is 9, above max_size 8"), (dict(flags=2), -1, "flags"), (dict(flags=3), -1, "flags"),
        (dict(cl_off=None), -1, "cl_size needs cl_off"), (dict(cl_off=None, cl_size=None), -1, "cl_first needs cl_off"),
        (dict(out_off=None), -1, "out_cloud needs out_off"), (dict(out_off=None, d_out=None), -1, "src_idx needs out_off"),
        (dict(d_out=O + 8), -1, "out_cloud must be 16-byte aligned"), (dict(src=S + 2), -1, "src_idx must be 4-byte aligned"), (dict(label=L + 2), -1, "label must be 4-byte aligned"),
        (dict(n=N + 1), -1, "n must be 4-byte aligned"), (dict(cl_size=CS + 2), -1, "cl_size must be 4-byte aligned"), (dict(cl_first=CF + 3), -1, "cl_first must be 4-byte aligned"),
        (dict(d_out=rec0 + 16), -1, "out_cloud overlaps the input clouds"), (dict(src=rec0), -1, "src_idx overlaps the input clouds"),
        (dict(label=rec0 + 4), -1, "label overlaps the input clouds"), (dict(kind=P + 16 * int(call.off[-1]) - 1), -1, "kind overlaps the input clouds"),
        (dict(n=rec0 + 8), -1, "n overlaps the input clouds"), (dict(cl_size=rec0 + 12), -1, "cl_size overlaps the input clouds"),
        (dict(cl_first=rec0), -1, "cl_first overlaps the input clouds"), (dict(src=O + 16), -1, "out_cloud overlaps src_idx"), (dict(kind=L + 1), -1, "label overlaps kind"),
        (dict(n=(K + 3) & ~3), -1, "kind overlaps n"), (dict(cl_size=N + 4), -1, "n overlaps cl_size"), (dict(cl_first=CS + 8), -1, "cl_size overlaps cl_first"),
        (dict(cl_first=O + 8), -1, "out_cloud overlaps cl_first"), (dict(label=S + 4), -1, "src_idx overlaps label"),
        (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31 records or more"),
    ]
    try:
        for change, code, word in refusals:
            out, coff, ooff = fresh_host_outputs(nc)
            kw = dict(base, out=out, cl_off=coff, out_off=ooff)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_cluster_dev, **kw)
            assert rc_ == code and word in msg and "lk_clouds_cluster_dev: " in msg, (change, rc_, msg)
            assert all(devguard.untouched(v.view(np.uint8)) for v in (out, coff, ooff)), change   # a refused call writes nothing
            call.gc.check()
            for (name, size, _), b in zip(OUTPUTS, call.buf):
                n = call.extent(name, good)
                raw = b.check()
                assert raw[:size * n].tobytes() == good[name].tobytes() and devguard.untouched(raw[size * n:]), (change, name)
        again = call.run()                                                                  # the handle is usable, a good call is right
        same(again, good, "after the refusals")
        # the host entry refuses the same way, under its own name (4-byte alignment for its clouds)
        hc = np.ascontiguousarray(call.rec)
        T = call.total
        u32 = lambda: np.zeros(T, dtype=np.uint32)                                          # noqa: E731
        hl, hk, hn, hs, hf, ho, hi = u32(), np.zeros(T, dtype=np.uint8), u32(), u32(), u32(), np.zeros((T, 4), dtype=np.float32), u32()
        hbase = dict(base, clouds=hc.ctypes.data, label=hl.ctypes.data, kind=hk.ctypes.data, n=hn.ctypes.data, cl_size=hs.ctypes.data, cl_first=hf.ctypes.data,
                     d_out=ho.ctypes.data, src=hi.ctypes.data)
        for change, code, word in ((dict(n_clouds=0), -1, "n_clouds"), (dict(reach=np.nan), -1, "reach"), (dict(clouds=hc.ctypes.data + 2), -1, "clouds must be 4-byte aligned"),
                                   (dict(min_pts=0), -1, "min_pts is 0"), (dict(min_size=2, max_size=1), -1, "min_size"), (dict(flags=4), -1, "flags"),
                                   (dict(out_off=None), -1, "out_off"), (dict(cl_off=None), -1, "cl_off"),
                                   (dict(label=hc.ctypes.data + 16 * LEAD), -1, "label overlaps the input clouds"), (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31")):
            out, coff, ooff = fresh_host_outputs(nc)
            kw = dict(hbase, out=out, cl_off=coff, out_off=ooff)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_cluster, **kw)
            assert rc_ == code and word in msg and "lk_clouds_cluster: " in msg, (change, rc_, msg)
            assert all(devguard.untouched(v.view(np.uint8)) for v in (out, coff, ooff)), change
            assert not any(v.any() for v in (hl, hk, hn, hs, hf, ho, hi)), change
        # a good call writes every byte of its n_clouds records and n_clouds + 1 offsets of either table and nothing behind them
        out, coff, ooff = fresh_host_outputs(nc)
        rc_, msg = raw_call(g, g.L.lk_clouds_cluster_dev, **dict(base, out=out, cl_off=coff, out_off=ooff, label=None, kind=None, n=None, cl_size=None, cl_first=None,
                                                                 d_out=None, src=None))
        assert rc_ == 0 and out[:nc].tobytes() == good["res"].tobytes() and devguard.untouched(out[nc:].view(np.uint8)), msg
        assert np.array_equal(ooff[:nc + 1], good["off"]) and devguard.untouched(ooff[nc + 1:].view(np.uint8))
        assert np.array_equal(coff[:nc + 1], good["cl_off"]) and devguard.untouched(coff[nc + 1:].view(np.uint8))
    finally:
        call.free()


def test_n_is_the_mme_count(g, main_group):
    """d_n == lk_clouds_mme_dev's d_n at the same radius, on the same clouds in the same buffer."""
    clouds, _ = with_nan_in_the_middle(main_group)
    call = Call(g, clouds, MAIN, want=(False, False, True, False, False, False, False))
    gn = devguard.Guarded(g, 4 * call.total, offset=4, name="cluster mme n")
    try:
        got = call.run()
        res = g.clouds_mme_dev(call.gc.ptr, call.off, cc.REACH, 5, gn.ptr)
        n = gn.read(np.uint32)
        ok = np.repeat(res["status"] == 0, np.diff(call.off.astype(np.int64)))
        assert ok.sum() > 1000 and np.array_equal(got["n"], n) and not n[~ok].any() and (n[ok] >= 1).all()
    finally:
        call.free(), gn.free()


def test_the_output_feeds_sor_and_mme_and_src_idx_gathers_the_input(g):
    """d_out / out_off go into lk_clouds_sor_dev and lk_clouds_mme_dev as they are, with the figures cloudmetrics gives on the filtered clouds; the
    input gathered through d_src_idx is d_out, and d_label at d_src_idx is a cluster of its cloud."""
    names = ["s257", "s0", "combs", "s255"]
    par = (cc.REACH, cc.MIN_PTS, 5, cc.NO_BOUND, 0)                               # clusters of fewer than five points go, and the noise
    clouds = [cc.CASES[n]["cloud"] for n in names]
    call = Call(g, clouds, par)
    try:
        got = call.run()
        off = got["off"]
        for i, name in enumerate(names):
            lo, hi = int(off[i]), int(off[i + 1])
            a, _ = call.span(i)
            assert np.array_equal(call.cloud_bits(i)[got["src"][lo:hi]], got["out"][lo:hi]), name
            lab = got["label"][a + got["src"][lo:hi].astype(np.int64)]
            assert (lab < int(got["res"][i]["n_clusters"])).all(), name                  # in bounds: never the noise label
            want = cloudmetrics.cluster(clouds[i], *par)
            assert np.array_equal(got["src"][lo:hi], want["src_idx"]) and int(got["res"][i]["n_kept"]) == want["n_kept"], name
        assert int(got["res"][0]["n_kept"]) == 243 + 5 and int(got["res"][0]["n_kept_clusters"]) == 2 and int(got["res"][0]["n_clusters"]) == 3
        filtered = [got["out"][int(off[i]):int(off[i + 1])].view(np.float32)[:, :3] for i in range(len(names))]
        d_out = call.buf[5].ptr
        mres = g.clouds_mme_dev(d_out, off, cc.REACH, 5)
        sres, _ = g.clouds_sor_dev(d_out, off, 4, cc.REACH, np.inf)
        call.buf[5].check(), call.gc.check()
        for i, name in enumerate(names):
            wm = cloudmetrics.mme(filtered[i], cc.REACH, 5)
            assert (int(mres[i]["n_points"]), int(mres[i]["n_dense"]), int(mres[i]["n_scored"]), int(mres[i]["n_pairs"])) == (len(filtered[i]), wm["n_dense"], wm["n_scored"],
                                                                                                                            wm["n_pairs"]), name
            ws = cloudmetrics.sor(filtered[i], 4, cc.REACH, np.inf)
            assert (int(sres[i]["n_points"]), int(sres[i]["n_isolated"]), int(sres[i]["n_kept"])) == (len(filtered[i]), ws["n_isolated"], ws["n_kept"]), name
    finally:
        call.free()


# ---- end to end: a run replayed on the frozen map, its registered cloud downsampled, a dense clump injected, the filters run where the cloud lies

@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def built():
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()


CLUMP_SEED = 1


def test_from_a_replay(built, oracle_lib, hip_lib, scene_plain):
    c = trr.build_case("plain", built, oracle_lib, hip_lib, scene_plain)
    runs, tbs, xs = c["runs"][:2], c["tbs"][:2], c["xs"][:2]
    t = hip_lib.flatten_runs(runs, tbs)
    n = len(t["pts"])
    file_off, _ = hip_lib.pcd_file_offsets(t["run_off"], t["scan_off"], 100)
    g = trr.new_handle(hip_lib, c["sc"], c["blob"], 2)
    d_pts = g.device_malloc(t["pts"].nbytes)
    gw = devguard.Guarded(g, 16 * n, offset=16, name="cluster replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="cluster replay d_out")
    call = scall = None
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * 2))
        g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, tmc.LEAF, go.ptr)
        assert not unf.any()
        a_len = int(out_off[1])
        cloud = np.frombuffer(go.check()[:16 * a_len].tobytes(), dtype=np.float32).reshape(a_len, 4)[:, :3]
        assert a_len > 5000
        # a dense clump of 60 points - a jittered 4 x 4 x 4 lattice at 0.8 leaf - beyond the cloud's corner, three reaches from everything, spread
        # through the records: locally as dense as the map, so the k-NN filter keeps it
        k, reach, min_pts = 8, 5.0 * tmc.LEAF, 4
        rng = np.random.default_rng(CLUMP_SEED)
        lattice = np.array([[x, y, z] for z in range(4) for y in range(4) for x in range(4)], dtype=np.float64)[:60] * (0.8 * tmc.LEAF)
        clump = (cloud.max(0).astype(np.float64) + 3.0 * reach + lattice + rng.uniform(-0.01, 0.01, size=lattice.shape)).astype(np.float32)
        at = np.linspace(0, a_len, 60, endpoint=False).astype(np.int64)
        mixed = np.insert(cloud, at, clump, axis=0)
        is_clump = np.zeros(len(mixed), dtype=bool)
        is_clump[at + np.arange(60)] = True
        assert np.array_equal(mixed[is_clump], clump)
        # every decision of the numpy statement clear of the reach by 2^10 float64 roundings, no point excused: membership, and the core point a
        # border point joins
        r2 = reach * reach
        pi, pj, pd = cloudmetrics.cluster_pairs(mixed, reach * (1.0 + 2.0 ** -20))
        clear = 1024.0 * 2.0 ** -53 * r2
        assert np.abs(pd - r2).min() >= clear, f"seed {CLUMP_SEED}: a pair lies at the reach"
        want = cloudmetrics.cluster(mixed, reach, min_pts, 0, cc.NO_BOUND, cc.KEEP_LARGEST)
        inside = pd <= r2
        core = want["kind"] == 2
        cand = inside & ~core[pi] & core[pj]
        order = np.lexsort((pd[cand], pi[cand]))
        bi, bd = pi[cand][order], pd[cand][order]
        second = np.flatnonzero(bi[1:] == bi[:-1]) + 1
        firsts = np.r_[True, bi[1:] != bi[:-1]] if len(bi) else np.zeros(0, dtype=bool)
        runner = second[firsts[second - 1]]                                       # the runner-up of each border point that has one
        assert not len(runner) or (bd[runner] - bd[runner - 1]).min() >= clear, f"seed {CLUMP_SEED}: a border point between two core points"
        # the clump passes the k-NN filter ...
        scall = tsg.Call(g, [mixed], k, reach, 2.0, tag="cluster replay sor")
        sgot = scall.run()
        assert sgot["keep"][is_clump].all() and (sgot["cnt"][is_clump] >= k).all()
        # ... and is gone after the largest component is kept
        call = Call(g, [mixed], (reach, min_pts, 0, cc.NO_BOUND, cc.KEEP_LARGEST), tag="cluster replay")
        got = call.run()
        r = got["res"][0]
        assert np.array_equal(got["label"], want["label"]) and np.array_equal(got["kind"], want["kind"]) and np.array_equal(got["n"], want["n"])   # no point excused
        assert np.array_equal(got["cl_size"], want["cl_size"]) and np.array_equal(got["cl_first"], want["cl_first"])
        assert np.array_equal(got["src"], want["src_idx"]) and np.array_equal(got["out"], call.cloud_bits(0)[want["keep"]])
        assert not np.isin(np.flatnonzero(is_clump), got["src"]).any() and len(set(got["label"][is_clump])) == 1 and (got["kind"][is_clump] == 2).all()
        assert int(r["n_kept"]) == int(r["largest_size"]) > 60 and int(r["n_kept_clusters"]) == 1 and int(r["n_clusters"]) >= 2 and int(r["status"]) == 0
        assert tuple(int(r[f]) for f in cc.COUNTS) == tuple(int(want[f]) for f in cc.COUNTS)
        print(f"\nreplay: map cloud of {a_len} points + a clump of 60 at reach = {reach}, min_pts = {min_pts}: clusters {int(r['n_clusters'])}, core {int(r['n_core'])}, "
              f"border {int(r['n_border'])}, noise {int(r['n_noise'])}, kept {int(r['n_kept'])}; nearest d2 to reach^2 {np.abs(pd - r2).min():.2e} m^2; the k-NN filter kept "
              f"{int(sgot['res'][0]['n_kept'])} points, the clump's 60 among them")
    finally:
        g.device_free(d_pts)
        gw.free(), go.free()
        for v in (call, scall):
            if v:
                v.free()
        g.close()
