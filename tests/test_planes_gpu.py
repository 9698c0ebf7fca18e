"""-m gpu: lk_clouds_planes_dev / lk_clouds_planes - the dominant planes peeled off many map clouds (RANSAC), on the device.

The cases are the frozen table of tests/planecloudcases.py, the expected values its exact evaluation (tests/golden/planecloud_cases.npz): labels,
counts, the winning hypotheses, the offsets, the output records and src_idx are whole numbers and are compared exactly; normal, d, centroid, eig and
rmse against the 50-digit values under planecloudcases.C_NORMAL / C_COORD.

Every call's clouds lie between the guard bands of tests/devguard.py at payload offset 16, behind three leading records of NaN that belong to nobody
(off[0] = 3); a cloud of NaN records sits in the middle of every call of several clouds; every record's w is a NaN with a payload of its own, so a
copy that is not bit for bit shows.  The outputs are guarded buffers of exactly off[n_clouds] - off[0] entries, so a write behind them lands in a
band, and what lies behind the kept records must still hold its fill."""
import ctypes as C
import itertools

import numpy as np
import pytest

import devguard
import planecloudcases as pc
import scenes
import test_map_clouds as tmc
import test_overlay_runs as tor
import test_replay_runs as trr
import test_sor_gpu as tsg
from legkilo_amd import abi, cloudmetrics

pytestmark = pytest.mark.gpu

GOLDEN = pc.golden()
REC = abi.planes_dtype()
PLANE = abi.plane_dtype()
LEAD = tsg.LEAD
NAN_CLOUD = tsg.NAN_CLOUD
records = tsg.records
OUTPUTS = (("label", 4, np.uint32), ("out", 16, np.uint8), ("src", 4, np.uint32))
ALL = (True,) * len(OUTPUTS)
NOTHING = (False,) * len(OUTPUTS)
MAIN = pc.MAIN


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
    """Clouds as ONE call in guarded device memory; want: which of OUTPUTS the call is given.  par: planecloudcases.PARAMS."""

    def __init__(self, g, clouds, par, want=ALL, tag="planes"):
        self.g, self.par = g, par
        self.rec, self.off = records(clouds)
        self.total = int(self.off[-1] - self.off[0])
        tag = f"{tag} {len(clouds)} {self.total}"
        self.gc = devguard.Guarded.input(g, self.rec, offset=16, name=tag + " clouds")
        self.buf = [devguard.Guarded(g, size * self.total, offset=size, name=f"{tag} {name}") if w else None for (name, size, _), w in zip(OUTPUTS, want)]

    def extent(self, name, got):
        return self.total if name == "label" else int(got["off"][-1])

    def run(self, want_off=None):
        """-> dict(res, planes, off (or None), and per output its array or None); bands untouched, the input unmodified, every entry of the documented
        extent written and nothing behind it."""
        dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags = self.par
        res, planes, off = self.g.clouds_planes_dev(self.gc.ptr, self.off, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags,
                                                    *[b.ptr if b else 0 for b in self.buf], want_off=want_off)
        self.gc.check()
        assert len(res) == len(self.off) - 1 and planes.shape == (len(res), max_planes)
        got = dict(res=res, planes=planes, off=off)
        for (name, size, dt), b in zip(OUTPUTS, self.buf):
            got[name] = None
            if b is None:
                continue
            raw = b.check()
            n = self.extent(name, got)
            assert devguard.untouched(raw[size * n:]), name                  # nothing behind the documented extent
            got[name] = np.frombuffer(raw[:size * n].tobytes(), dtype=np.uint32).reshape(n, 4) if name == "out" else np.frombuffer(raw[:size * n].tobytes(), dtype=dt)
            assert not n or name == "label" or devguard.sentinel_free(got[name]), name   # (0xffffffff is the label of a point on no plane)
        if off is not None:
            assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), res["n_kept"].astype(np.int64))
        assert not res["pad"].any()
        for k in range(len(res)):                                           # unused plane entries are zero, every byte
            assert not planes[k, int(res[k]["n_planes"]):].view(np.uint8).any(), k
            assert int(planes[k]["n_inliers"].sum()) == int(res[k]["n_on_planes"])
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


def run_once(g, clouds, par, want=ALL, tag="planes", **kw):
    c = Call(g, clouds, par, want, tag)
    try:
        return c, c.run(**kw)
    finally:
        c.free()


def with_nan_in_the_middle(names):
    """-> (clouds, index of each name's cloud)"""
    clouds = [pc.CASES[n]["cloud"] for n in names]
    if len(names) < 2:
        return clouds, list(range(len(names)))
    mid = len(names) // 2
    return clouds[:mid] + [NAN_CLOUD] + clouds[mid:], [i if i < mid else i + 1 for i in range(len(names))]


def cut(call, got, k):
    """cloud k's part of a call's results: (record, planes, label, out, src)"""
    a, b = call.span(k)
    lo, hi = int(got["off"][k]), int(got["off"][k + 1])
    return got["res"][k], got["planes"][k], got["label"][a:b], got["out"][lo:hi], got["src"][lo:hi]


def check_case(name, bits, part, worst):
    """every whole number exactly, the coefficients within the bounds"""
    rec, planes, label, out, src = part
    c, want = pc.CASES[name], GOLDEN[name]
    assert int(rec["n_points"]) == len(c["cloud"]) and all(int(rec[f]) == want[f] for f in pc.COUNTS), (name, rec, {f: want[f] for f in pc.COUNTS})
    k = want["n_planes"]
    assert np.array_equal(label, want["label"]) and planes["n_inliers"][:k].tolist() == want["n_inliers"].tolist() and planes["hyp"][:k].tolist() == want["hyp"].tolist(), name
    kept = np.flatnonzero(want["keep"])
    assert np.array_equal(src, kept) and np.array_equal(out, bits[kept]), name       # input order, all 16 bytes, w's payload included
    assert want["status"] or int(rec["n_points"]) == int(rec["n_on_planes"]) + int(rec["n_rest"]), name
    en, ec = pc.coefficient_errors(c["cloud"], want, [planes[r] for r in range(k)])
    worst[0], worst[1] = max(worst[0], en), max(worst[1], ec)
    assert en <= pc.C_NORMAL and ec <= pc.C_COORD, (name, en, ec)


def nan_part_is_empty(part):
    rec, planes, label, out, src = part
    assert int(rec["status"]) == abi.LK_PLANES_NONFINITE and int(rec["n_points"]) == len(label)
    assert not any(int(rec[f]) for f in pc.COUNTS if f != "status") and not planes.view(np.uint8).any()
    assert (label == abi.LK_PLANES_NONE).all() and len(out) == len(src) == 0


def same(a, b, want):
    assert a["res"].tobytes() == b["res"].tobytes() and a["planes"].tobytes() == b["planes"].tobytes(), want
    for name, _, _ in OUTPUTS:
        assert a[name] is None or a[name].tobytes() == b[name].tobytes(), (want, name)
    assert a["off"] is None or np.array_equal(a["off"], b["off"]), want


def test_every_case_in_one_call_and_alone_and_twice(g):
    worst = [0.0, 0.0]
    for par, names in pc.groups().items():
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
            check_case(name, call.cloud_bits(i), part, worst)
            _, one = run_once(g, [pc.CASES[name]["cloud"]], par)
            assert one["res"][0].tobytes() == part[0].tobytes() and one["planes"][0].tobytes() == part[1].tobytes(), name   # the same bits whatever else the call holds
            assert one["label"].tobytes() == part[2].tobytes() and np.array_equal(one["out"][:, :3], part[3][:, :3]) and np.array_equal(one["src"], part[4]), name
    i, j = (pc.groups()[MAIN].index(n) for n in ("twin_a", "twin_b"))
    print(f"\ndevice: normal within {worst[0]:.3f}, centroid / d / eig / rmse^2 within {worst[1]:.3f} units of 2^-53 * scale (bounds {pc.C_NORMAL}, {pc.C_COORD})")
    assert j == i + 1


def test_two_clouds_with_the_same_coordinates_give_the_same_bits(g):
    names = pc.groups()[MAIN]
    clouds, at = with_nan_in_the_middle(names)
    call, got = run_once(g, clouds, MAIN)
    a, b = (cut(call, got, at[names.index(n)]) for n in ("twin_a", "twin_b"))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[4], b[4])
    assert np.array_equal(a[3][:, :3], b[3][:, :3]) and not np.array_equal(a[3][:, 3], b[3][:, 3])        # (each with its own w)
    # placement: the same cloud at (3000, 2000, 100) - the decisions use differences, the labels do not move
    o, f = (cut(call, got, at[names.index(n)]) for n in ("place_origin", "place_far"))
    assert o[2].tobytes() == f[2].tobytes() and o[1]["hyp"].tolist() == f[1]["hyp"].tolist() and o[1]["n_inliers"].tolist() == f[1]["n_inliers"].tolist()


@pytest.fixture(scope="module")
def main_group():
    return pc.groups()[MAIN]


def test_null_outputs_host_entry_and_poisoned_pools(g, hip_lib, main_group, clean_env):
    clouds, _ = with_nan_in_the_middle(main_group)
    _, full = run_once(g, clouds, MAIN)
    for want in itertools.product((False, True), repeat=len(OUTPUTS)):  # every subset of the optional outputs NULL: the same bits
        if not all(want):
            same(run_once(g, clouds, MAIN, want=want)[1], full, want)
    _, tables = run_once(g, clouds, MAIN, want=NOTHING, want_off=True)                       # the offset table alone
    assert tables["res"].tobytes() == full["res"].tobytes() and np.array_equal(tables["off"], full["off"])
    rec, roff = records(clouds)
    h = g.clouds_planes(rec, roff, *MAIN)
    assert h["res"].tobytes() == full["res"].tobytes() and h["planes"].tobytes() == full["planes"].tobytes() and np.array_equal(h["out_off"], full["off"])
    assert np.array_equal(h["out"].view(np.uint32), full["out"]) and np.array_equal(h["src_idx"], full["src"]) and np.array_equal(h["label"], full["label"])
    # the other kept set: the points on planes
    keep = MAIN[:7] + (abi.LK_PLANES_KEEP_PLANES,)
    call, kp = run_once(g, clouds, keep)
    assert kp["planes"].tobytes() == full["planes"].tobytes() and kp["label"].tobytes() == full["label"].tobytes()
    assert np.array_equal(kp["res"]["n_kept"], full["res"]["n_on_planes"]) and int(kp["off"][-1]) + int(full["off"][-1]) == int((full["res"]["status"] == 0) @ full["res"]["n_points"])
    for k in range(len(clouds)):
        lo, hi = int(kp["off"][k]), int(kp["off"][k + 1])
        assert np.array_equal(kp["src"][lo:hi], np.flatnonzero(full["label"][slice(*call.span(k))] != abi.LK_PLANES_NONE)), k
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        for want in (ALL, NOTHING, (True, False, False), (False, True, False)):
            same(run_once(gp, clouds, MAIN, want=want)[1], full, want)
        hp = gp.clouds_planes(rec, roff, *MAIN)
        assert hp["res"].tobytes() == full["res"].tobytes() and hp["planes"].tobytes() == full["planes"].tobytes()
    finally:
        gp.close()


def test_status_clouds_leave_their_neighbours_alone(g, main_group):
    """The group's call with and without the two non-finite cases: every other cloud keeps its bits, and a status cloud comes out empty."""
    bad = ["nan_cloud", "inf_cloud"]
    assert all(b in main_group for b in bad)
    a, ga = run_once(g, [pc.CASES[n]["cloud"] for n in main_group], MAIN)
    b, gb = run_once(g, [pc.CASES[n]["cloud"] for n in main_group if n not in bad], MAIN)
    keep_i = [i for i, n in enumerate(main_group) if n not in bad]
    assert ga["res"][keep_i].tobytes() == gb["res"].tobytes() and ga["planes"][keep_i].tobytes() == gb["planes"].tobytes()
    for j, i in enumerate(keep_i):
        pa, pb = cut(a, ga, i), cut(b, gb, j)
        assert np.array_equal(pa[3][:, :3], pb[3][:, :3]) and pa[2].tobytes() == pb[2].tobytes() and pa[4].tobytes() == pb[4].tobytes(), main_group[i]
    for i, name in enumerate(main_group):
        if name in bad:
            part = cut(a, ga, i)
            nan_part_is_empty(part)
            assert int(part[0]["n_points"]) == 60
    names = ["range_at", "range_below"]                                          # out of range: |coordinate| at 2^30, and one float below
    call, got = run_once(g, [pc.CASES[n]["cloud"] for n in names], pc.params(pc.CASES["range_at"]))
    assert got["res"]["status"].tolist() == [abi.LK_PLANES_RANGE, 0] and got["off"].tolist() == [0, 0, 1] and got["res"]["n_planes"].tolist() == [0, 1]
    assert (got["label"][:4] == abi.LK_PLANES_NONE).all() and sorted(got["label"][4:].tolist()) == [0, 0, 0, abi.LK_PLANES_NONE] and int(got["res"][0]["n_points"]) == 4


def raw_call(g, fn, clouds, n_clouds, off, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, out, planes, label, d_out, out_off, src):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = fn(g.h, ptr(clouds), C.c_size_t(n_clouds), arr(off), C.c_double(dist), C.c_uint32(n_hyp), C.c_uint32(max_planes), C.c_uint32(min_inliers), arr(axis),
             C.c_double(cos_max_angle), C.c_uint64(seed), C.c_uint32(flags), arr(out), arr(planes), ptr(label), ptr(d_out), arr(out_off), ptr(src))
    return rc_, g.L.lk_last_error(g.h).decode()


def fresh_host_outputs(nc, max_planes):
    return (np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC), np.full((nc + 1) * max_planes, 0xFF, dtype=np.uint8).repeat(PLANE.itemsize).view(PLANE),
            np.full(nc + 3, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))


def test_refusals(g):
    names = ["s65", "twin_a", "s2"]
    call = Call(g, [pc.CASES[n]["cloud"] for n in names], MAIN)
    good = call.run()
    nc = len(names)
    P = call.gc.ptr
    L, O, S = (b.ptr for b in call.buf)
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                           # noqa: E731
    f64 = lambda *v: np.array(v, dtype=np.float64)                                          # noqa: E731
    base = dict(clouds=P, n_clouds=nc, off=call.off, dist=MAIN[0], n_hyp=MAIN[1], max_planes=MAIN[2], min_inliers=MAIN[3], axis=None, cos_max_angle=MAIN[5], seed=MAIN[6],
                flags=MAIN[7], label=L, d_out=O, src=S)
    dec = call.off.copy()
    dec[1] = dec[2] + 1
    rec0 = P + 16 * int(call.off[0])
    refusals = [
        (dict(n_clouds=0), -1, "n_clouds"), (dict(clouds=None), -1, "null argument (clouds)"), (dict(off=None), -1, "null argument (off)"),
        (dict(out=None), -1, "null argument (out)"), (dict(planes=None), -1, "null argument (planes)"), (dict(clouds=P + 8), -1, "clouds must be 16-byte aligned"),
        (dict(off=dec), -1, "off decreases at cloud 1"),
        (dict(dist=0.0), -1, "dist"), (dict(dist=-1.0), -1, "dist"), (dict(dist=np.nan), -1, "dist"), (dict(dist=np.inf), -1, "dist"),
        (dict(n_hyp=0), -1, "n_hyp is 0"), (dict(n_hyp=4097), -1, "n_hyp is 4097"), (dict(max_planes=0), -1, "max_planes is 0"), (dict(max_planes=17), -1, "max_planes is 17"),
        (dict(min_inliers=2), -1, "min_inliers is 2"), (dict(min_inliers=0), -1, "min_inliers is 0"),
        (dict(axis=f64(0.0, 0.0, 0.0)), -1, "axis"), (dict(axis=f64(0.0, np.nan, 1.0)), -1, "axis"), (dict(axis=f64(np.inf, 0.0, 1.0)), -1, "axis"),
        (dict(cos_max_angle=-0.5), -1, "cos_max_angle"), (dict(cos_max_angle=1.5), -1, "cos_max_angle"), (dict(cos_max_angle=np.nan), -1, "cos_max_angle"),
        (dict(flags=2), -1, "flags"), (dict(flags=3), -1, "flags"),
        (dict(out_off=None), -1, "out_cloud needs out_off"), (dict(out_off=None, d_out=None), -1, "src_idx needs out_off"),
        (dict(d_out=O + 8), -1, "out_cloud must be 16-byte aligned"), (dict(src=S + 2), -1, "src_idx must be 4-byte aligned"), (dict(label=L + 2), -1, "label must be 4-byte aligned"),
        (dict(d_out=rec0 + 16), -1, "out_cloud overlaps the input clouds"), (dict(src=rec0), -1, "src_idx overlaps the input clouds"),
        (dict(label=rec0 + 4), -1, "label overlaps the input clouds"), (dict(src=O + 16), -1, "out_cloud overlaps src_idx"), (dict(label=S + 4), -1, "src_idx overlaps label"),
        (dict(label=O + 32), -1, "out_cloud overlaps label"),
        (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31 records or more"),
    ]
    try:
        for change, code, word in refusals:
            out, planes, ooff = fresh_host_outputs(nc, MAIN[2])
            kw = dict(base, out=out, planes=planes, out_off=ooff)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_planes_dev, **kw)
            assert rc_ == code and word in msg and "lk_clouds_planes_dev: " in msg, (change, rc_, msg)
            assert all(devguard.untouched(v.view(np.uint8)) for v in (out, planes, ooff)), change   # a refused call writes nothing
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
        hl, ho, hi = np.zeros(T, dtype=np.uint32), np.zeros((T, 4), dtype=np.float32), np.zeros(T, dtype=np.uint32)
        hbase = dict(base, clouds=hc.ctypes.data, label=hl.ctypes.data, d_out=ho.ctypes.data, src=hi.ctypes.data)
        for change, code, word in ((dict(n_clouds=0), -1, "n_clouds"), (dict(dist=np.nan), -1, "dist"), (dict(clouds=hc.ctypes.data + 2), -1, "clouds must be 4-byte aligned"),
                                   (dict(n_hyp=0), -1, "n_hyp is 0"), (dict(max_planes=17), -1, "max_planes"), (dict(min_inliers=1), -1, "min_inliers"), (dict(flags=4), -1, "flags"),
                                   (dict(axis=f64(0.0, 0.0, 0.0)), -1, "axis"), (dict(cos_max_angle=2.0), -1, "cos_max_angle"), (dict(out_off=None), -1, "out_off"),
                                   (dict(planes=None), -1, "planes"),
                                   (dict(label=hc.ctypes.data + 16 * LEAD), -1, "label overlaps the input clouds"), (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31")):
            out, planes, ooff = fresh_host_outputs(nc, MAIN[2])
            kw = dict(hbase, out=out, planes=planes, out_off=ooff)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_planes, **kw)
            assert rc_ == code and word in msg and "lk_clouds_planes: " in msg, (change, rc_, msg)
            assert all(devguard.untouched(v.view(np.uint8)) for v in (out, planes, ooff)), change
            assert not any(v.any() for v in (hl, ho, hi)), change
        # a good call writes every byte of its n_clouds records, its n_clouds * max_planes plane records and n_clouds + 1 offsets and nothing behind them
        out, planes, ooff = fresh_host_outputs(nc, MAIN[2])
        rc_, msg = raw_call(g, g.L.lk_clouds_planes_dev, **dict(base, out=out, planes=planes, out_off=ooff, label=None, d_out=None, src=None))
        assert rc_ == 0 and out[:nc].tobytes() == good["res"].tobytes() and devguard.untouched(out[nc:].view(np.uint8)), msg
        assert planes[:nc * MAIN[2]].tobytes() == good["planes"].tobytes() and devguard.untouched(planes[nc * MAIN[2]:].view(np.uint8))
        assert np.array_equal(ooff[:nc + 1], good["off"]) and devguard.untouched(ooff[nc + 1:].view(np.uint8))
    finally:
        call.free()


def floor_with_objects():
    """A floor of 40 x 40 points at 0.125 and three 4 x 4 x 4 blocks that stand on it, 0.125 above it and well apart; shuffled."""
    u = 0.125
    floor = np.array([[x * u, y * u, 0.0] for y in range(40) for x in range(40)])
    block = np.array([[x * u, y * u, (z + 1) * u] for z in range(4) for y in range(4) for x in range(4)])
    pts = np.r_[floor, block + [0.5, 0.5, 0.0], block + [2.5, 1.0, 0.0], block + [1.0, 3.5, 0.0]]
    return pts[np.random.default_rng(7).permutation(len(pts))].astype(np.float32)


def test_the_remainder_feeds_clustering(g):
    """d_out / out_off of a floor-plus-objects cloud go into lk_clouds_cluster_dev as they are: the objects as separate clusters with the numpy
    statement's counts, where the unfiltered cloud is one cluster."""
    cloud = floor_with_objects()
    par = (0.03125, 64, 1, 500, (0.0, 0.0, 1.0), pc.COS10, 5, 0)
    reach = 0.1875
    want = cloudmetrics.planes(cloud, *par)
    assert want["n_planes"] == 1 and want["planes"][0]["n_inliers"] == 1600 and want["n_rest"] == 192
    clouds = [cloud, pc.CASES["s0"]["cloud"], cloud[::-1]]
    call = Call(g, clouds, par)
    try:
        got = call.run()
        off = got["off"]
        assert got["res"]["n_planes"].tolist() == [1, 0, 1] and off.tolist() == [0, 192, 192, 384]
        assert np.array_equal(got["src"][:192], want["src_idx"]) and np.array_equal(got["out"][:192], call.cloud_bits(0)[want["keep"]])
        assert np.array_equal(got["label"][:len(cloud)], want["label"]) and abs(float(got["planes"][0, 0]["normal"][2]) - 1.0) < 1e-12 and float(got["planes"][0, 0]["rmse"]) < 1e-12
        whole, _, _ = g.clouds_cluster_dev(call.gc.ptr, call.off, reach, 1)
        parts, _, _ = g.clouds_cluster_dev(call.buf[1].ptr, off, reach, 1)
        call.buf[1].check(), call.gc.check()
        rest = cloudmetrics.cluster(cloud[want["keep"]], reach, 1)
        assert whole["n_clusters"].tolist() == [1, 0, 1] and cloudmetrics.cluster(cloud, reach, 1)["n_clusters"] == 1          # everything stands on the floor
        assert parts["n_clusters"].tolist() == [3, 0, 3] and rest["n_clusters"] == 3 and rest["cl_size"].tolist() == [64, 64, 64]
        assert (int(parts[0]["n_core"]), int(parts[0]["largest_size"]), int(parts[0]["n_points"])) == (rest["n_core"], rest["largest_size"], 192)
    finally:
        call.free()


# ---- end to end: a run replayed on the frozen map, its registered cloud downsampled, the planes peeled off where the cloud lies

@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def built():
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()


REPLAY = (0.05, 128, 3, 200, None, 0.0, 20261021, 0)      # dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags


def test_from_a_replay(built, oracle_lib, hip_lib, scene_plain):
    c = trr.build_case("plain", built, oracle_lib, hip_lib, scene_plain)
    runs, tbs, xs = c["runs"][:2], c["tbs"][:2], c["xs"][:2]
    t = hip_lib.flatten_runs(runs, tbs)
    n = len(t["pts"])
    file_off, _ = hip_lib.pcd_file_offsets(t["run_off"], t["scan_off"], 100)
    g = trr.new_handle(hip_lib, c["sc"], c["blob"], 2)
    d_pts = g.device_malloc(t["pts"].nbytes)
    gw = devguard.Guarded(g, 16 * n, offset=16, name="planes replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="planes replay d_out")
    call = None
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * 2))
        g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, tmc.LEAF, go.ptr)
        assert not unf.any()
        a_len = int(out_off[1])
        cloud = np.frombuffer(go.check()[:16 * a_len].tobytes(), dtype=np.float32).reshape(a_len, 4)[:, :3].copy()
        assert a_len > 5000
        trace = []
        want = cloudmetrics.planes(cloud, *REPLAY, trace=trace)
        gap = min(r[4] for r in trace)
        assert gap > 2.0 ** -40, f"seed {REPLAY[6]}: a record lies at the threshold ({gap:.3e})"      # every decision of the numpy statement is clear, no point excused
        call = Call(g, [cloud], REPLAY, tag="planes replay")
        got = call.run()
        r = got["res"][0]
        assert np.array_equal(got["label"], want["label"]) and np.array_equal(got["src"], want["src_idx"]) and np.array_equal(got["out"], call.cloud_bits(0)[want["keep"]])
        k = want["n_planes"]
        assert k >= 1 and got["planes"][0]["hyp"][:k].tolist() == [p["hyp"] for p in want["planes"]] and got["planes"][0]["n_inliers"][:k].tolist() == [p["n_inliers"] for p in want["planes"]]
        assert tuple(int(r[f]) for f in pc.COUNTS) == tuple(int(want[f]) for f in pc.COUNTS) and int(r["n_points"]) == a_len
        for j, p in enumerate(want["planes"]):                                                       # the coefficients: two float64 routes, a loose bound of their own
            dev = got["planes"][0][j]
            assert np.abs(np.asarray(dev["normal"]) - p["normal"]).max() < 1e-9 and abs(float(dev["d"]) - p["d"]) < 1e-8 and abs(float(dev["rmse"]) - p["rmse"]) < 1e-9
        print(f"\nreplay: map cloud of {a_len} points at dist = {REPLAY[0]}, n_hyp = {REPLAY[1]}: planes {k} with {[p['n_inliers'] for p in want['planes']]} inliers, "
              f"rmse {[round(p['rmse'], 4) for p in want['planes']]}, rest {int(r['n_rest'])}; smallest |s*s - t2q| / t2q {gap:.3e}")
    finally:
        g.device_free(d_pts)
        gw.free(), go.free()
        if call:
            call.free()
        g.close()
