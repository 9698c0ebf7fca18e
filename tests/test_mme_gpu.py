"""-m gpu: lk_clouds_mme_dev / lk_clouds_mme - mean map entropy and mean plane variance of many clouds, on the device.

The cases are the frozen table of tests/mmecases.py, the expected values its exact / 50-digit evaluation (tests/golden/mme_cases.npz): n_i, the class
of every point, the counts, worst and status are compared exactly, h / lmin and the records' figures within the bounds derived there.

Every call's clouds lie between the guard bands of tests/devguard.py at payload offset 16, behind three leading records of NaN that belong to nobody
(off[0] != 0); a cloud of NaN records sits in the middle of every call of several clouds; every record's w is NaN (never read).  The per-point arrays
are guarded outputs of exactly off[n_clouds] - off[0] entries, so a write behind them lands in a band."""
import ctypes as C
import itertools

import numpy as np
import pytest

import devguard
import mmecases as mc
import scenes
import test_map_clouds as tmc
import test_overlay_runs as tor
import test_replay_runs as trr
from legkilo_amd import abi, cloudmetrics

pytestmark = pytest.mark.gpu

GOLDEN = mc.golden()
REC = abi.mme_dtype()
LEAD = 3
NAN_CLOUD = np.full((5, 3), np.nan, dtype=np.float32)


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
    """Clouds [n_i, 3] as one buffer of x y z w records behind `lead` records of NaN, w = NaN -> (float32 [N, 4], offsets uint64 [len(clouds) + 1])."""
    parts = [np.full((lead, 3), np.nan, dtype=np.float32)] + [np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds]
    xyz = np.concatenate(parts)
    rec = np.full((len(xyz), 4), np.nan, dtype=np.float32)
    rec[:, :3] = xyz
    return rec, (lead + np.r_[0, np.cumsum([len(p) for p in parts[1:]])]).astype(np.uint64)


class Call:
    """Clouds as ONE call in guarded device memory; want = (n, h, lmin): which per-point outputs the call is given."""

    def __init__(self, g, clouds, radius, min_pts, want=(True, True, True), tag="mme"):
        self.g, self.radius, self.min_pts = g, radius, min_pts
        self.rec, self.off = records(clouds)
        self.total = int(self.off[-1] - self.off[0])
        tag = f"{tag} {len(clouds)} {self.total}"
        self.gc = devguard.Guarded.input(g, self.rec, offset=16, name=tag + " clouds")
        self.out = [devguard.Guarded(g, size * self.total, offset=size, name=f"{tag} {k}") if w else None for k, size, w in zip("nhl", (4, 8, 8), want)]

    def run(self):
        """-> (records, n, h, lmin), None for an output not asked for; bands untouched, the input unmodified, every entry written."""
        res = self.g.clouds_mme_dev(self.gc.ptr, self.off, self.radius, self.min_pts, *[b.ptr if b else 0 for b in self.out])
        self.gc.check()
        assert len(res) == len(self.off) - 1
        arrays = [b.read(dt) if b else None for b, dt in zip(self.out, (np.uint32, np.float64, np.float64))]
        for a in arrays:
            assert a is None or (len(a) == self.total and (not self.total or devguard.sentinel_free(a)))
        return (res, *arrays)

    def span(self, k):
        return int(self.off[k] - self.off[0]), int(self.off[k + 1] - self.off[0])

    def free(self):
        for b in [self.gc] + self.out:
            if b:
                b.free()


def with_nan_in_the_middle(names):
    """-> (clouds, index of each name's cloud)"""
    clouds = [mc.CASES[n]["cloud"] for n in names]
    if len(names) < 2:
        return clouds, list(range(len(names)))
    mid = len(names) // 2
    return clouds[:mid] + [NAN_CLOUD] + clouds[mid:], [i if i < mid else i + 1 for i in range(len(names))]


def check_case(name, rec, n, h, lmin, ratios):
    """Decisions exactly, figures within tolerance; ratios: [worst h ratio, worst lmin ratio] against the bounds at C = 1, updated."""
    c, want = mc.CASES[name], GOLDEN[name]
    assert int(rec["status"]) == want["status"] and int(rec["n_points"]) == len(c["cloud"]), name
    assert (int(rec["n_dense"]), int(rec["n_scored"]), int(rec["n_pairs"]), int(rec["worst"])) == (want["n_dense"], want["n_scored"], want["n_pairs"], want["worst"]), name
    assert np.array_equal(n, want["n"]), name
    cls = np.where(np.isnan(lmin), mc.SPARSE, np.where(np.isnan(h), mc.FLAT, mc.SCORED))
    assert np.array_equal(cls, want["cls"]), name
    sc, de = want["cls"] == mc.SCORED, want["cls"] != mc.SPARSE
    eh, el = np.abs(h[sc] - want["h"][sc]), np.abs(lmin[de] - want["lmin"][de])
    th, tl = mc.tol_h(want, 1.0)[sc], mc.tol_lmin(c, 1.0)
    if sc.any():
        print(f"{name}: h ratio {(eh / th).max():.2f}", end="  ")
        ratios[0] = max(ratios[0], float((eh / th).max()))
    if de.any():
        print(f"{name}: lmin ratio {el.max() / tl:.2f}")
        ratios[1] = max(ratios[1], float(el.max() / tl))
    assert (eh <= mc.C_H * th).all() and (el <= mc.C_L * tl).all(), name
    for f, t in zip(mc.FIGURES, mc.tol_record(c, want)):
        assert np.isnan(rec[f]) == np.isnan(want[f]), (name, f)
        if not np.isnan(want[f]):
            assert abs(float(rec[f]) - want[f]) <= t, (name, f, float(rec[f]), want[f], t)
    if want["n_scored"]:
        assert float(rec["h_max"]) == h[want["worst"]], name


def test_every_case_in_one_call_and_alone(g):
    ratios = [0.0, 0.0]
    for (radius, min_pts), names in mc.groups().items():
        clouds, at = with_nan_in_the_middle(names)
        many = Call(g, clouds, radius, min_pts)
        try:
            res, n, h, lmin = many.run()
            spans = [many.span(k) for k in at]
            if len(names) > 1:
                k = len(names) // 2
                a, b = many.span(k)
                assert int(res[k]["status"]) == abi.LK_MME_NONFINITE and not n[a:b].any() and np.isnan(h[a:b]).all() and np.isnan(lmin[a:b]).all()
        finally:
            many.free()
        for name, k, (a, b) in zip(names, at, spans):
            check_case(name, res[k], n[a:b], h[a:b], lmin[a:b], ratios)
            alone = Call(g, [mc.CASES[name]["cloud"]], radius, min_pts)
            try:
                r1, n1, h1, l1 = alone.run()
            finally:
                alone.free()
            assert r1[0].tobytes() == res[k].tobytes(), name        # a cloud's record has the same bits whatever else the call holds
            assert np.array_equal(n1, n[a:b]) and h1.tobytes() == h[a:b].tobytes() and l1.tobytes() == lmin[a:b].tobytes(), name
    print(f"\ndevice: worst ratio h {ratios[0]:.3f} (C_H {mc.C_H}), lmin {ratios[1]:.3f} (C_L {mc.C_L})")


@pytest.fixture(scope="module")
def main_group():
    return mc.groups()[(mc.R, mc.MIN_PTS)]


def test_null_outputs_host_entry_and_poisoned_pools(g, hip_lib, main_group, clean_env):
    clouds, _ = with_nan_in_the_middle(main_group)
    full = Call(g, clouds, mc.R, mc.MIN_PTS)
    try:
        res, n, h, lmin = full.run()
    finally:
        full.free()
    ref = (n, h, lmin)
    for want in itertools.product((False, True), repeat=3):          # every combination of NULL per-point outputs: the same bits
        if all(want):
            continue
        part = Call(g, clouds, mc.R, mc.MIN_PTS, want)
        try:
            got = part.run()
        finally:
            part.free()
        assert got[0].tobytes() == res.tobytes(), want
        for a, b in zip(got[1:], ref):
            assert a is None or a.tobytes() == b.tobytes(), want
    rec, off = records(clouds)
    hres, hn, hh, hl = g.clouds_mme(rec, off, mc.R, mc.MIN_PTS, want_points=True)
    assert hres.tobytes() == res.tobytes() and np.array_equal(hn, n) and hh.tobytes() == h.tobytes() and hl.tobytes() == lmin.tobytes()
    assert g.clouds_mme(rec, off, mc.R, mc.MIN_PTS).tobytes() == res.tobytes()
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    gp = tmc.new_handle(hip_lib)
    try:
        for want in ((True, True, True), (False, False, False)):
            p = Call(gp, clouds, mc.R, mc.MIN_PTS, want)
            try:
                got = p.run()
            finally:
                p.free()
            assert got[0].tobytes() == res.tobytes()
            for a, b in zip(got[1:], ref):
                assert a is None or a.tobytes() == b.tobytes()
        assert gp.clouds_mme(rec, off, mc.R, mc.MIN_PTS).tobytes() == res.tobytes()
    finally:
        gp.close()


def test_status_clouds_leave_their_neighbours_alone(g, main_group):
    """The group's call with and without the two non-finite cases: every other cloud keeps its bits."""
    bad = ["nan_cloud", "inf_cloud"]
    assert all(b in main_group for b in bad)
    a = Call(g, [mc.CASES[n]["cloud"] for n in main_group], mc.R, mc.MIN_PTS)
    b = Call(g, [mc.CASES[n]["cloud"] for n in main_group if n not in bad], mc.R, mc.MIN_PTS)
    try:
        ra, na, ha, la = a.run()
        rb, nb, hb, lb = b.run()
        keep = [i for i, n in enumerate(main_group) if n not in bad]
        pick = lambda v: np.concatenate([v[slice(*a.span(i))] for i in keep])   # noqa: E731
        assert ra[keep].tobytes() == rb.tobytes()
        assert np.array_equal(pick(na), nb) and pick(ha).tobytes() == hb.tobytes() and pick(la).tobytes() == lb.tobytes()
        for i, name in enumerate(main_group):
            if name in bad:
                r, (lo, hi) = ra[i], a.span(i)
                assert int(r["status"]) == abi.LK_MME_NONFINITE and all(np.isnan(r[f]) for f in mc.FIGURES) and int(r["n_points"]) == 60
                assert (int(r["n_dense"]), int(r["n_scored"]), int(r["n_pairs"]), int(r["worst"])) == (0, 0, 0, 0)
                assert not na[lo:hi].any() and np.isnan(ha[lo:hi]).all() and np.isnan(la[lo:hi]).all()
    finally:
        a.free(), b.free()
    names = ["range_at", "range_below"]                                          # out of range: its own group (radius 2^-10)
    c = Call(g, [mc.CASES[n]["cloud"] for n in names], mc.CASES["range_at"]["radius"], mc.MIN_PTS)
    try:
        r, n, h, lmin = c.run()
    finally:
        c.free()
    assert r["status"].tolist() == [abi.LK_MME_RANGE, 0] and n.tolist() == [0, 0, 0] + GOLDEN["range_below"]["n"].tolist() and int(r[0]["n_points"]) == 3


def raw_call(g, fn, clouds, n_clouds, off, radius, min_pts, out, n, h, lmin):
    ptr = lambda v: None if v is None else C.c_void_p(v)                                    # noqa: E731
    arr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                     # noqa: E731
    rc_ = fn(g.h, ptr(clouds), C.c_size_t(n_clouds), arr(off), C.c_double(radius), C.c_uint32(min_pts), arr(out), ptr(n), ptr(h), ptr(lmin))
    return rc_, g.L.lk_last_error(g.h).decode()


def test_refusals(g):
    names = ["s65", "duplicates", "s5"]
    call = Call(g, [mc.CASES[n]["cloud"] for n in names], mc.R, mc.MIN_PTS)
    good, good_n, good_h, good_l = call.run()
    nc = len(names)
    P, N, H, L = call.gc.ptr, call.out[0].ptr, call.out[1].ptr, call.out[2].ptr
    base = dict(clouds=P, n_clouds=nc, off=call.off, radius=mc.R, min_pts=mc.MIN_PTS, n=N, h=H, lmin=L)
    dec = call.off.copy()
    dec[1] = dec[2] + 1
    u64 = lambda *v: np.array(v, dtype=np.uint64)                                           # noqa: E731
    rec0 = P + 16 * int(call.off[0])
    refusals = [
        (dict(n_clouds=0), -1, "n_clouds"), (dict(clouds=None), -1, "null argument (clouds)"), (dict(off=None), -1, "null argument (off)"),
        (dict(out=None), -1, "null argument (out)"), (dict(clouds=P + 8), -1, "clouds must be 16-byte aligned"), (dict(n=N + 2), -1, "n must be 4-byte aligned"),
        (dict(h=H + 4), -1, "h must be 8-byte aligned"), (dict(lmin=L + 4), -1, "lmin must be 8-byte aligned"), (dict(off=dec), -1, "off decreases at cloud 1"),
        (dict(radius=0.0), -1, "radius"), (dict(radius=-1.0), -1, "radius"), (dict(radius=np.nan), -1, "radius"), (dict(radius=np.inf), -1, "radius"),
        (dict(min_pts=3), -1, "min_pts is 3"), (dict(min_pts=0), -1, "min_pts is 0"),
        (dict(n=rec0 + 16), -1, "n overlaps the input clouds"), (dict(h=P + 16 * int(call.off[-1]) - 8), -1, "h overlaps the input clouds"),
        (dict(lmin=rec0), -1, "lmin overlaps the input clouds"), (dict(n=H + 8), -1, "n overlaps h"), (dict(lmin=H), -1, "h overlaps lmin"), (dict(lmin=N + 4), -1, "n overlaps lmin"),
        (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31 records or more"), (dict(off=u64(0, 0xffffffff, 0xffffffff, 0xffffffff)), -3, "2^31 records or more"),
    ]
    try:
        for change, code, word in refusals:
            out = np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
            kw = dict(base, out=out)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_mme_dev, **kw)
            assert rc_ == code and word in msg and "lk_clouds_mme_dev: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)), change                          # a refused call writes nothing
            call.gc.check()
            assert call.out[0].check().tobytes() == good_n.tobytes() and call.out[1].check().tobytes() == good_h.tobytes(), change
            assert call.out[2].check().tobytes() == good_l.tobytes(), change
            again = call.run()                                                             # the handle is usable, a good call is right
            assert again[0].tobytes() == good.tobytes() and again[2].tobytes() == good_h.tobytes(), change
        # the host entry refuses the same way, under its own name (4-byte alignment for its clouds)
        hc = np.ascontiguousarray(call.rec)
        hn, hh, hl = np.zeros(call.total, dtype=np.uint32), np.zeros(call.total), np.zeros(call.total)
        hbase = dict(base, clouds=hc.ctypes.data, n=hn.ctypes.data, h=hh.ctypes.data, lmin=hl.ctypes.data)
        for change, code, word in ((dict(n_clouds=0), -1, "n_clouds"), (dict(radius=np.nan), -1, "radius"), (dict(clouds=hc.ctypes.data + 2), -1, "clouds must be 4-byte aligned"),
                                   (dict(min_pts=3), -1, "min_pts"), (dict(h=hc.ctypes.data + 16 * LEAD), -1, "h overlaps the input clouds"),
                                   (dict(off=u64(0, 1, 2, 1 << 31)), -3, "2^31")):
            out = np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
            kw = dict(hbase, out=out)
            kw.update(change)
            rc_, msg = raw_call(g, g.L.lk_clouds_mme, **kw)
            assert rc_ == code and word in msg and "lk_clouds_mme: " in msg, (change, rc_, msg)
            assert devguard.untouched(out.view(np.uint8)) and not hn.any() and not hh.any() and not hl.any(), change
        # a good call writes every byte of its n_clouds records and nothing behind them
        out = np.full(nc + 2, 0xFF, dtype=np.uint8).repeat(REC.itemsize).view(REC)
        rc_, msg = raw_call(g, g.L.lk_clouds_mme_dev, **dict(base, out=out, n=None, h=None, lmin=None))
        assert rc_ == 0 and out[:nc].tobytes() == good.tobytes() and devguard.untouched(out[nc:].view(np.uint8)), msg
    finally:
        call.free()


def test_a_shift_by_1024_m_keeps_every_bit(g):
    """Coordinates that are multiples of 2^-10 and r = 0.25: a shift by exactly 1024 m per axis keeps every float exact and moves every cell by 4096,
    so the keys, the order and every offset about a query point are the same - and so is every bit of the result.  Sums about the origin would not
    survive this."""
    base = np.round(mc.CASES["s257"]["cloud"].astype(np.float64) * 1024.0) / 1024.0
    shifted = (base + 1024.0).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64) - 1024.0, base) and np.array_equal(base.astype(np.float32).astype(np.float64), base)
    out = []
    for cloud in (base, shifted):
        c = Call(g, [cloud], mc.R, mc.MIN_PTS, tag="mme shift")
        try:
            out.append(c.run())
        finally:
            c.free()
    (r0, n0, h0, l0), (r1, n1, h1, l1) = out
    assert int(r0[0]["n_scored"]) > 200
    assert r0.tobytes() == r1.tobytes() and np.array_equal(n0, n1) and h0.tobytes() == h1.tobytes() and l0.tobytes() == l1.tobytes()
    want = cloudmetrics.mme(base, mc.R, mc.MIN_PTS)
    assert np.array_equal(n0, want["n"]) and int(r0[0]["n_scored"]) == want["n_scored"]


def test_a_shuffled_cloud_gives_the_same_points(g):
    rng = np.random.default_rng(5)
    for name in ("s257", "duplicates", "tilted_plane_1mm"):
        c, want = mc.CASES[name], GOLDEN[name]
        perm = rng.permutation(len(c["cloud"]))
        call = Call(g, [c["cloud"][perm]], c["radius"], c["min_pts"], tag="mme shuffle")
        try:
            res, n, h, lmin = call.run()
        finally:
            call.free()
        back = np.empty_like(perm)
        back[perm] = np.arange(len(perm))
        n, h, lmin = n[back], h[back], lmin[back]                    # entry i = the figures of the table's point i
        assert np.array_equal(n, want["n"]), name
        assert np.array_equal(np.isnan(h), want["cls"] != mc.SCORED) and np.array_equal(np.isnan(lmin), want["cls"] == mc.SPARSE), name
        sc, de = want["cls"] == mc.SCORED, want["cls"] != mc.SPARSE
        assert (np.abs(h[sc] - want["h"][sc]) <= mc.tol_h(want)[sc]).all() and (np.abs(lmin[de] - want["lmin"][de]) <= mc.tol_lmin(c)).all(), name
        assert (int(res[0]["n_dense"]), int(res[0]["n_scored"]), int(res[0]["n_pairs"])) == (want["n_dense"], want["n_scored"], want["n_pairs"]), name
        assert perm[int(res[0]["worst"])] == want["worst"] or np.array_equal(c["cloud"][perm[int(res[0]["worst"])]], c["cloud"][want["worst"]]), name
        for f, t in zip(mc.FIGURES, mc.tol_record(c, want)):
            assert abs(float(res[0][f]) - want[f]) <= t, (name, f)


# ---- end to end: two runs replayed on the frozen map, their registered clouds downsampled, the map clouds scored where they lie

@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def built():
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()


def kappa_of(cloud, radius):
    """(tr / 3)^3 / det of every point's covariance, from cloudmetrics.mme_moments (NaN or inf where the point has none)"""
    n, s, m = cloudmetrics.mme_moments(cloud, radius)
    nn = np.maximum(n.astype(np.float64), 2.0)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    c = [(m[:, k] - s[:, i] * s[:, j] / nn) / (nn - 1.0) for k, (i, j) in enumerate(pairs)]
    det = (c[0] * (c[3] * c[5] - c[4] * c[4]) - c[1] * (c[1] * c[5] - c[4] * c[2])) + c[2] * (c[1] * c[4] - c[3] * c[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (((c[0] + c[3]) + c[5]) / 3.0) ** 3 / det


def test_from_a_replay(built, oracle_lib, hip_lib, scene_plain):
    c = trr.build_case("plain", built, oracle_lib, hip_lib, scene_plain)
    runs, tbs, xs = c["runs"][:2], c["tbs"][:2], c["xs"][:2]   # runs of 3 scans and of 1
    t = hip_lib.flatten_runs(runs, tbs)
    n = len(t["pts"])
    file_off, file_run = hip_lib.pcd_file_offsets(t["run_off"], t["scan_off"], 100)
    assert file_run.tolist() == [0, 1]
    g = trr.new_handle(hip_lib, c["sc"], c["blob"], 2)
    d_pts = g.device_malloc(t["pts"].nbytes)
    gw = devguard.Guarded(g, 16 * n, offset=16, name="mme replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="mme replay d_out")
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * 2))
        _, sbo = g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, tmc.LEAF, go.ptr)
        m = int(out_off[-1])
        assert not unf.any() and m > 100
        img = go.check().copy()
        clouds = np.frombuffer(img[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        B = int(sbo[-1])
        before = (g.batch_get_states(0, 2), trr.times_of(g, 2), g.runs_bucket_poses(0, B).tobytes(), g.map_export().copy())
        radius = 5.0 * tmc.LEAF
        gn, gh, gl = (devguard.Guarded(g, s * m, offset=s, name=f"mme replay {k}") for k, s in zip("nhl", (4, 8, 8)))
        try:
            res = g.clouds_mme_dev(go.ptr, out_off, radius, 5, gn.ptr, gh.ptr, gl.ptr)
            assert go.check().tobytes() == img.tobytes(), "the call changed the map clouds"
            cnt, h, lmin = gn.read(np.uint32), gh.read(np.float64), gl.read(np.float64)
        finally:
            gn.free(), gh.free(), gl.free()
        for k in range(2):
            lo, hi = int(out_off[k]), int(out_off[k + 1])
            want = cloudmetrics.mme(clouds[lo:hi, :3], radius, 5)
            assert np.array_equal(cnt[lo:hi], want["n"]), k
            assert np.array_equal(np.isnan(h[lo:hi]), ~want["scored"]) and np.array_equal(np.isnan(lmin[lo:hi]), ~want["dense"]), k
            r = res[k]
            assert (int(r["status"]), int(r["n_points"]), int(r["n_dense"]), int(r["n_scored"]), int(r["n_pairs"])) == (0, hi - lo, want["n_dense"], want["n_scored"],
                                                                                                                      want["n_pairs"]), k
            # either side lies within its bound of the truth: twice the bound, kappa from the numpy statement's own covariances
            kap = kappa_of(clouds[lo:hi, :3], radius)
            sc, de = want["scored"], want["dense"]
            th = 2 * mc.C_H * mc.ULP * (kap + np.abs(want["h"]))
            tl = 2 * mc.tol_lmin(dict(radius=radius))
            assert (np.abs(h[lo:hi][sc] - want["h"][sc]) <= th[sc]).all() and (np.abs(lmin[lo:hi][de] - want["lmin"][de]) <= tl).all(), k
            if want["n_scored"]:
                assert abs(float(r["mme"]) - want["mme"]) <= th[sc].mean() and abs(float(r["mpv"]) - want["mpv"]) <= tl, k
                assert float(r["h_max"]) == h[lo:hi][int(r["worst"])] == np.nanmax(h[lo:hi]), k
        print(f"replay: map clouds of {int(out_off[1])} and {m - int(out_off[1])} points at r = {radius}: dense {res['n_dense'].tolist()}, scored "
              f"{res['n_scored'].tolist()}, mme {res['mme'].tolist()}, mpv {res['mpv'].tolist()}")
        assert int(res["n_dense"].sum()) > 0
        # the slots, the bucket table and the map are as they were
        after = (g.batch_get_states(0, 2), trr.times_of(g, 2), g.runs_bucket_poses(0, B).tobytes(), g.map_export())
        assert np.array_equal(after[0][0], before[0][0]) and np.array_equal(after[0][1], before[0][1]) and after[1] == before[1]
        assert after[2] == before[2] and np.array_equal(after[3], before[3])
    finally:
        g.device_free(d_pts)
        gw.free()
        go.free()
        g.close()
