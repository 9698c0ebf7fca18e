"""The lidar front end on the crafted clouds of tests/cloudcases.py: rounding halves, -0.0, the blind sphere, cell faces, denormals, the grid
limit, ties of the time sort, equal cell keys across a scan boundary.  Every comparison is on BITS (bytes / uint32 / uint64 views): `==` on
floats cannot tell -0.0 from +0.0.

CPU   the reference's own handlers == po.decode on every decode case (the oracle is right AT these edges, not only between them);
      po.voxel_grid_centroid == its loop form == a float64-carried restatement written here; po.decode_vec == po.decode; and "the table
      bites": every wrong variant of the arithmetic, restated here, differs from the oracle on a named case - a device kernel with that fault
      would fail the GPU tests below.
GPU   lk_decode_scan_dev / lk_preprocess_scan_dev / lk_decode_scans_dev (between guard bands) and the host wrappers on every case they apply to.
"""
import functools
import math
import struct

import numpy as np
import pytest

import cloudcases as cc
import oracle_binding as ob
import preprocess_oracle as po
import scenes
from devguard import Guarded
from legkilo_amd import synth

F32 = np.float32
PT = synth.POINT_DTYPE.itemsize
SMALL = dict(max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12)   # test_lidar_frontend.py's
FIELDS = ("x", "y", "z", "curvature")


def dbits(v):
    return struct.pack("<d", float(v))


def assert_same_points(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in FIELDS:
        a, b = np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, f, int(bad.size), int(bad[0]), float(got[f][bad[0]]), float(want[f][bad[0]]))


def same_points(got, want):
    return len(got) == len(want) and all(np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes() for f in FIELDS)


_DECODED = {}


def oracle_decode(raw, lidar_type, time_scale, filter_num, blind, header_stamp):
    """po.decode, computed once per (message, parameters): the table's arrays are shared between the cases and the runs."""
    key = (id(raw), lidar_type, time_scale, filter_num, blind, header_stamp)
    if key not in _DECODED:
        _DECODED[key] = (raw, po.decode(raw, lidar_type, time_scale, filter_num, blind, header_stamp=header_stamp))
    return _DECODED[key][1]


def case_decode(c):
    return oracle_decode(c.raw, c.lidar_type, c.time_scale, c.filter_num, c.blind, c.header_stamp)


@functools.lru_cache(maxsize=None)
def oracle_grid(name):
    c = cc.grid_case(name)
    return po.preprocess(c.pts, c.leaf)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """Per message of a batch case: (decoded + filtered + sorted scan, begin, end) from the oracle."""
    b = next(x for x in cc.BATCH_CASES if x.name == name)
    out = []
    for s, t in enumerate(cc.run_stamps(len(b.msgs))):
        dec, tb, te = oracle_decode(b.msgs[s], b.lidar_type, b.time_scale, b.filter_num, b.blind, float(t))
        out.append((po.preprocess(dec, b.leaf), tb, te))
    return out


# ------------------------------------------------------------------------------------------------------------- restatements (float64-carried)
def c_round(v):
    """std::round of a double: half away from zero, the sign kept (also of a zero result)."""
    a = abs(v)
    fl = math.floor(a)
    return math.copysign(fl + (1.0 if a - fl >= 0.5 else 0.0), v)      # a - fl is exact


def restated_decode(c, half_even=False, drop_sign=False, blind_ge=False, fused=False):
    """The three handlers with every product, sum and quotient taken in float64 and, where the handler works in float, rounded to float32
    straight after.  The keyword arguments are FAULTS: round half to even; the magnitude rounded without restoring the sign; >= in the blind
    check; the blind sum contracted into fused multiply-adds."""
    raw, lt = c.raw, c.lidar_type
    tt = np.float64(c.time_scale) * raw[cc.TNAME[lt]].astype(np.float64)
    if lt != 3:
        tt = tt.astype(F32)
    b2 = F32(F32(c.blind) * F32(c.blind))
    out = []
    for i in range(len(raw)):
        x, y, z = F32(raw["x"][i]), F32(raw["y"][i]), F32(raw["z"][i])
        s = cc.sumsq_fused(x, y, z) if fused else cc.sumsq(x, y, z)
        if i % c.filter_num or (b2 >= s if blind_ge else b2 > s):
            continue
        v = float((tt[i] - tt[0]) * 500.0) if lt == 3 else float(F32(float(F32(float(tt[i]) - float(tt[0]))) * 500.0))
        r = float(np.rint(v)) if half_even else abs(c_round(v)) if drop_sign else c_round(v)
        out.append((x, y, z, F32(r / 500.0)))       # Hesai: a double quotient cast to float; the others: a float quotient (innocuous through float64)
    base = 0.0 if lt == 3 else c.header_stamp
    return np.array(out, dtype=po.OUT_DTYPE), base + float(tt[0]), base + float(tt[-1])


def _rows(pts, flush=False):
    """lk_points as Python floats (float64 carriers of the float32 values)."""
    rows = [[float(p[f]) for f in FIELDS] for p in pts]
    if flush:
        tiny = float(np.finfo(F32).tiny)
        rows = [[math.copysign(0.0, v) if abs(v) < tiny else v for v in r] for r in rows]
    return rows


def _keys(rows, leaf, trunc=False, min_first=False):
    """Cell ids as Python ints: ijk = floor(float32(p * inv)) - min_b, id = i + j * div0 + k * div0 * div1.  p * inv is exact in float64."""
    inv = float(F32(1.0 / float(F32(leaf))))
    cell = (lambda v: math.trunc(float(F32(v * inv)))) if trunc else (lambda v: math.floor(float(F32(v * inv))))
    mn = [cell(rows[0][a] if min_first else min(r[a] for r in rows)) for a in range(3)]
    dv = [cell(max(r[a] for r in rows)) - mn[a] + 1 for a in range(3)]
    return [(cell(r[0]) - mn[0]) + (cell(r[1]) - mn[1]) * dv[0] + (cell(r[2]) - mn[2]) * dv[0] * dv[1] for r in rows]


def _sum32(v, order):
    if order == "pairwise":
        if len(v) <= 2:
            return float(F32(v[0] + v[1])) if len(v) == 2 else v[0]
        return float(F32(_sum32(v[:len(v) // 2], order) + _sum32(v[len(v) // 2:], order)))
    acc = 0.0
    for a in (v[::-1] if order == "reverse" else v):
        acc = float(F32(acc + a))
    return acc


def _centroid(group, order="seq"):
    return [float(F32(_sum32([r[a] for r in group], order) / float(len(group)))) for a in range(4)]


def _time_sort(cells, ties="asc", raw_bits=False):
    idx = range(len(cells))
    if raw_bits:
        key = lambda i: int(F32(cells[i][3]).view(np.uint32))      # noqa: E731
    elif ties == "desc":
        key = lambda i: (cells[i][3], -i)                          # noqa: E731
    else:
        key = lambda i: cells[i][3]                                # noqa: E731  (-0.0 == +0.0: one time; sorted() is stable)
    return [cells[i] for i in sorted(idx, key=key)]


def _as_points(cells):
    out = np.zeros(len(cells), dtype=synth.POINT_DTYPE)
    for a, f in enumerate(FIELDS):
        out[f] = np.array([c[a] for c in cells], dtype=np.float64).astype(F32)      # exact: every value is a float32
    return out


def restated_grid(pts, leaf, trunc=False, flush=False, min_first=False, order="seq"):
    """Cells in ascending id, each the float32 centroid of its points summed in input order.  FAULTS: truncation instead of floor; denormals
    flushed to zero on input; min_b from the first point; sums in reverse order / pairwise."""
    rows = _rows(pts, flush)
    cells = {}
    for k, r in zip(_keys(rows, leaf, trunc, min_first), rows):
        cells.setdefault(k & 0xFFFFFFFF if min_first else k, []).append(r)      # the faulty ids are negative: as unsigned 32-bit sort keys they wrap
    return [_centroid(cells[k], order) for k in sorted(cells)]


def restated_preprocess(pts, leaf, ties="asc", raw_bits=False, **faults):
    return _as_points(_time_sort(restated_grid(pts, leaf, **faults), ties, raw_bits))


def restated_run(clouds, leaf, scan_boundary=True):
    """lk_decode_scans_dev's cell build over the decoded scans of a run: the scans' points sorted by cell id back to back, a new cell wherever
    the id changes and - scan_boundary - wherever the scan does; scan s owns the cells from the rank of its first point's head on.
    FAULT: heads from id changes only."""
    keys, rows, sid = [], [], []
    for s, pts in enumerate(clouds):
        r = _rows(pts)
        k = _keys(r, leaf)
        for i in sorted(range(len(r)), key=lambda i: k[i]):
            keys.append(k[i]), rows.append(r[i]), sid.append(s)
    head = [i == 0 or keys[i] != keys[i - 1] or (scan_boundary and sid[i] != sid[i - 1]) for i in range(len(keys))]
    starts = [i for i, h in enumerate(head) if h] + [len(keys)]
    cells = [_centroid(rows[a:b]) for a, b in zip(starts[:-1], starts[1:])]
    rank = np.r_[0, np.cumsum(head)]
    first = [sid.index(s) for s in range(len(clouds))]
    off = [int(rank[i]) for i in first] + [len(cells)]
    return [_as_points(_time_sort(cells[off[s]:off[s + 1]])) for s in range(len(clouds))]


# ------------------------------------------------------------------------------------------------------------- CPU
def test_the_table_is_complete():
    names = {c.name.split("[")[0] for c in cc.DECODE_CASES}
    assert names >= {"halves", "minus_zero", "blind_edge", "blind0", "filter_ge_n", "filter_n_minus_1", "first_blind", "ouster_large_t", "scaled",
                     "odd_layout"}
    for lt in (1, 2, 3):
        assert {c.name for c in cc.DECODE_CASES if c.lidar_type == lt} >= {f"{n}[{lt}]" for n in ("halves", "minus_zero", "blind_edge", "blind0",
                                                                                                     "filter_ge_n", "odd_layout")}
    for leaf in cc.LEAVES:
        assert {g.name for g in cc.GRID_CASES} >= {f"{n}[{leaf}]" for n in ("faces_x", "faces_y", "faces_z", "faces_xyz", "zeros_min_denormal",
                                                                              "zeros_min_negzero", "zeros_min_m5", "order_visible", "stamps")}
    assert {"under_limit", "over_limit"} <= {g.name for g in cc.GRID_CASES}
    batch = {b.name.split("[")[0].rstrip("0123456789").rstrip("_") for b in cc.BATCH_CASES}
    assert batch >= {"collapsed_run", "equal_key_boundary", "many_messages", "all_cases_one_run", "over_limit_run"}
    assert sorted(len(b.msgs) for b in cc.BATCH_CASES if b.name.startswith("many_messages")) == [1, 255, 256, 257]
    # the stated counts (cloudcases asserts them too, at import)
    for lt in (1, 2):
        assert sum(v[0] for k, v in cc.HALVES.items() if k[1] == lt and k[0] != "scaled") >= 20
        assert sum(v[1] for k, v in cc.HALVES.items() if k[1] == lt and k[0] != "scaled") >= 20
    assert cc.HALVES[("halves", 3)] == (2, 2) and sum(cc.HALVES[("halves_first_0.25", 3)]) >= 20
    assert all(len(cc.BLIND_POINTS[k]) >= 10 for k in ("eq", "under", "over", "straddle"))
    assert all(min(v) >= 10 for v in cc.ORDER_VISIBLE.values())


@pytest.mark.skipif(ob.build_ref() is None, reason="oracle/_ref not built and the reference sources absent")
def test_reference_decode_equals_the_oracle_on_every_decode_case():
    """The reference's handlers, compiled unmodified (oracle/_ref), against po.decode: the bits of x, y, z, curvature.  begin / end go through
    a `float` temporary that g++ -O3 keeps in double for the Ouster handler (tests/test_reference_pin.py::test_decode_matches_the_reference),
    so they are compared to float precision - the only tolerance in this file."""
    for c in cc.DECODE_CASES:
        want, wb, we = case_decode(c)
        got, gb, ge = ob.ref_decode(c.raw, c.layout, c.time_scale, c.filter_num, c.blind, header_stamp=c.header_stamp)
        assert_same_points(got, want, c.name)
        assert abs(gb - wb) <= 1e-7 * max(1.0, abs(wb)) and abs(ge - we) <= 1e-7 * max(1.0, abs(we)), (c.name, gb, wb, ge, we)


def test_decode_restatement_and_vectorised_form_equal_the_oracle():
    for c in cc.DECODE_CASES:
        want, wb, we = case_decode(c)
        got, gb, ge = restated_decode(c)
        assert_same_points(got, want, c.name)
        assert (dbits(gb), dbits(ge)) == (dbits(wb), dbits(we)), c.name
        if c.lidar_type in (1, 2):
            vec, vb, ve = po.decode_vec(c.raw, c.lidar_type, c.time_scale, c.filter_num, c.blind, header_stamp=c.header_stamp)
            assert_same_points(vec, want, c.name + " (decode_vec)")
            assert (dbits(vb), dbits(ve)) == (dbits(wb), dbits(we)), c.name


def test_decode_cases_hit_their_edges_in_the_oracle():
    """What the cases claim, read off the ORACLE's output: halves round away from zero on both sides, -0.0 appears, the points on the blind
    sphere are kept and those one ulp inside dropped, filter_num and the blind first point keep what they should."""
    for lt in (1, 2, 3):
        dec = case_decode(cc.decode_case(f"minus_zero[{lt}]"))[0]
        neg = np.signbit(dec["curvature"]) & (dec["curvature"] == 0)
        assert neg.sum() >= 4 and (~np.signbit(dec["curvature"]) & (dec["curvature"] == 0)).sum() >= 4, lt
        c = cc.decode_case(f"blind_edge[{lt}]")
        dec = case_decode(c)[0]
        kept = {(float(p["x"]), float(p["y"]), float(p["z"])) for p in dec}
        for kind, keep in (("eq", True), ("over", True), ("under", False)):
            assert all((tuple(map(float, p)) in kept) == keep for p in cc.BLIND_POINTS[kind]), (lt, kind)
        assert len(case_decode(cc.decode_case(f"blind0[{lt}]"))[0]) == 5
        assert len(case_decode(cc.decode_case(f"filter_ge_n[{lt}]"))[0]) == 1 and len(case_decode(cc.decode_case(f"filter_n_minus_1[{lt}]"))[0]) == 2
        c = cc.decode_case(f"first_blind[{lt}]")
        dec, tb, te = case_decode(c)
        assert len(dec) == len(c.raw) - 1 and np.all(dec["curvature"] < 0) and te < tb
        c = cc.decode_case(f"halves[{lt}]")
        dec = case_decode(c)[0]
        v = cc.scaled_offset(lt, c.time_scale, c.raw[cc.TNAME[lt]], c.raw[cc.TNAME[lt]][0])
        half = np.abs(v) % 1 == 0.5
        assert half.sum() >= 4
        want = (np.sign(v[half]) * (np.abs(v[half]) + 0.5) / 500.0).astype(F32) if lt == 3 else \
            ((np.sign(v[half]) * (np.abs(v[half]) + F32(0.5))).astype(F32) / F32(500.0)).astype(F32)
        assert dec["curvature"][half].tobytes() == want.tobytes(), lt


def test_grid_oracle_equals_its_loop_form_and_the_float64_restatement():
    for g in cc.GRID_CASES:
        a = po.voxel_grid_centroid(g.pts, g.leaf)
        b = po.voxel_grid_centroid_loops(g.pts, g.leaf)
        assert_same_points(b, a, g.name + " (loops)")
        assert_same_points(_as_points(restated_grid(g.pts, g.leaf)), a, g.name + " (restated cells)")
        assert_same_points(restated_preprocess(g.pts, g.leaf), po.preprocess(g.pts, g.leaf), g.name + " (restated, sorted)")
    for leaf in cc.LEAVES:
        srt = oracle_grid(f"stamps[{leaf}]")
        z = np.flatnonzero(srt["curvature"] == 0)
        assert np.signbit(srt["curvature"][z]).any() and not np.signbit(srt["curvature"][z[0]])    # a -0.0 stamp, and not at the head of its tie run


def _decoded_clouds(b):
    return [oracle_decode(m, b.lidar_type, b.time_scale, b.filter_num, b.blind, float(t))[0] for m, t in zip(b.msgs, cc.run_stamps(len(b.msgs)))]


def test_the_table_bites():
    """Each wrong variant differs from the oracle, on bits, on at least one case - named here."""
    report = {}
    decode_faults = {"round half to even": dict(half_even=True), "magnitude rounded, sign not restored": dict(drop_sign=True),
                     ">= in the blind check": dict(blind_ge=True), "fused x*x+y*y+z*z": dict(fused=True)}
    for fault, kw in decode_faults.items():
        cases = [c for c in cc.DECODE_CASES if "fused" not in kw or c.name.startswith("blind")]     # exact fused sums are slow: the blind cases only
        report[fault] = [c.name for c in cases if not same_points(restated_decode(c, **kw)[0], case_decode(c)[0])]
    grid_faults = {"truncation instead of floor": dict(trunc=True), "denormals flushed to zero on input": dict(flush=True),
                   "min_b from the first point": dict(min_first=True), "centroid sums in reverse order": dict(order="reverse"),
                   "centroid sums pairwise": dict(order="pairwise"), "time sort: ties by descending cell": dict(ties="desc"),
                   "time sort on the raw bit pattern": dict(raw_bits=True)}
    for fault, kw in grid_faults.items():
        report[fault] = [g.name for g in cc.GRID_CASES if not same_points(restated_preprocess(g.pts, g.leaf, **kw), po.preprocess(g.pts, g.leaf))]
    fault = "cell heads from key changes only (no scan boundary)"
    report[fault] = []
    for b in cc.BATCH_CASES:
        if b.lidar_type == 1 and b.name.split("[")[0] in ("collapsed_run", "equal_key_boundary"):
            clouds, want = _decoded_clouds(b), [w[0] for w in oracle_run(b.name)]
            assert all(same_points(a, w) for a, w in zip(restated_run(clouds, b.leaf), want)), b.name     # the fault-free restatement is the oracle
            if not all(same_points(a, w) for a, w in zip(restated_run(clouds, b.leaf, scan_boundary=False), want)):
                report[fault].append(b.name)
    expect = {"round half to even": "halves", "magnitude rounded, sign not restored": "halves", ">= in the blind check": "blind_edge",
              "fused x*x+y*y+z*z": "blind_edge", "truncation instead of floor": "faces", "denormals flushed to zero on input": "zeros",
              "min_b from the first point": "zeros_min_m5", "centroid sums in reverse order": "order_visible",
              "centroid sums pairwise": "order_visible", "time sort: ties by descending cell": "stamps", "time sort on the raw bit pattern": "stamps",
              fault: "collapsed_run"}
    for f, names in report.items():
        print(f"{f}: differs on {', '.join(names) if names else 'NOTHING'}")
    assert set(report) == set(expect)
    for f, names in report.items():
        assert any(n.startswith(expect[f]) for n in names), (f, names)
    assert any(n.startswith("equal_key_boundary") for n in report[fault]) and any(n.startswith("blind0") for n in report[">= in the blind check"])
    assert any(n.startswith("minus_zero") for n in report["magnitude rounded, sign not restored"])


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def scene():
    return scenes.Scene(**SMALL)


def _decode_dev(g, c):
    d_msg = Guarded.input(g, c.raw.view(np.uint8), offset=1, name="d_msg_data")
    d_out = Guarded(g, len(c.raw) * PT, offset=16, name="d_out")
    try:
        n_out, tb, te = g.decode_scan_dev(d_msg.ptr, len(c.raw), c.layout, c.time_scale, c.filter_num, c.blind, c.header_stamp, d_out.ptr)
        d_msg.check()
        return d_out.read(synth.POINT_DTYPE, n_out), tb, te
    finally:
        d_msg.free()
        d_out.free()


def _preprocess_dev(g, pts, leaf):
    d_raw = Guarded.input(g, pts, offset=16, name="d_raw")
    d_out = Guarded(g, len(pts) * PT, offset=48, name="d_out_sorted")
    try:
        n_out = g.preprocess_scan_dev(d_raw.ptr, len(pts), leaf, d_out.ptr)
        d_raw.check()
        return d_out.read(synth.POINT_DTYPE, n_out)
    finally:
        d_raw.free()
        d_out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_decode_scan_dev_on_every_decode_case(hip_lib, scene, lidar_type):
    g = hip_lib.LegKiloHip(scene.cfg())
    try:
        for c in cc.DECODE_CASES:
            if c.lidar_type == lidar_type:
                want, wb, we = case_decode(c)
                got, tb, te = _decode_dev(g, c)
                assert_same_points(got, want, c.name)
                assert (dbits(tb), dbits(te)) == (dbits(wb), dbits(we)), (c.name, tb, wb, te, we)
    finally:
        g.close()


@pytest.mark.gpu
def test_preprocess_scan_dev_on_every_grid_case(hip_lib, scene):
    """Every grid case (under_limit included) equals the oracle; over_limit is refused and the same handle then runs `faces` correctly."""
    g = hip_lib.LegKiloHip(scene.cfg())
    try:
        for c in cc.GRID_CASES:
            if c.refused:
                with pytest.raises(hip_lib.LegKiloError, match=r"error -1: .*leaf too small"):
                    _preprocess_dev(g, c.pts, c.leaf)
                for name in ("faces_xyz[0.5]", "faces_xyz[0.3]"):
                    assert_same_points(_preprocess_dev(g, cc.grid_case(name).pts, cc.grid_case(name).leaf), oracle_grid(name), name + " after the refusal")
            else:
                assert_same_points(_preprocess_dev(g, c.pts, c.leaf), oracle_grid(c.name), c.name)
        assert [c.name for c in cc.GRID_CASES if c.refused] == ["over_limit"]
    finally:
        g.close()


class _Run:
    """A packed run between guard bands, output room for the batch entry, scratch for the per-scan chain."""

    def __init__(self, g, b, seed):
        self.g, self.b = g, b
        self.buf, self.msg_off, self.n_points = synth.pack_cloud_run(b.msgs, seed=seed)
        self.stamps = cc.run_stamps(len(b.msgs))
        self.d_msgs = Guarded.input(g, self.buf, offset=1, name="d_msgs")
        self.d_out = Guarded(g, int(self.n_points.sum()) * PT, offset=16, name="d_out")
        self.d_dec = g.device_malloc(int(self.n_points.max()) * PT)
        self.d_ds = g.device_malloc(int(self.n_points.max()) * PT)

    def batch(self):
        b = self.b
        so, tb, te = self.g.decode_scans_dev(self.d_msgs.ptr, self.msg_off, self.n_points, self.stamps, b.layout, b.time_scale, b.filter_num, b.blind,
                                             b.leaf, self.d_out.ptr)
        self.d_msgs.check()
        out = self.d_out.read(synth.POINT_DTYPE, int(so[-1]))
        return [out[int(so[s]):int(so[s + 1])] for s in range(len(so) - 1)], tb, te, so

    def chain(self, s):
        b = self.b
        n, tb, te = self.g.decode_scan_dev(self.d_msgs.ptr + int(self.msg_off[s]), int(self.n_points[s]), b.layout, b.time_scale, b.filter_num, b.blind,
                                           float(self.stamps[s]), self.d_dec)
        nd = self.g.preprocess_scan_dev(self.d_dec, n, b.leaf, self.d_ds)
        o = np.zeros(nd, dtype=synth.POINT_DTYPE)
        self.g.d2h(o, self.d_ds)
        return o, tb, te

    def free(self):
        self.d_msgs.free(), self.d_out.free()
        self.g.device_free(self.d_dec), self.g.device_free(self.d_ds)


def _assert_run(g, b, seed):
    """The batch entry on run b == the per-scan chain on the same device bytes == the oracle; scan_off exact, begin / end on bits."""
    want = oracle_run(b.name)
    r = _Run(g, b, seed)
    try:
        got, tb, te, so = r.batch()
        assert [int(v) for v in so] == [0] + [int(v) for v in np.cumsum([len(w[0]) for w in want])], b.name
        for s, (w, wb, we) in enumerate(want):
            assert_same_points(got[s], w, (b.name, s, "oracle"))
            assert (dbits(tb[s]), dbits(te[s])) == (dbits(wb), dbits(we)), (b.name, s, tb[s], wb, te[s], we)
        for s in range(len(want)):
            o, cb, ce = r.chain(s)
            assert got[s].tobytes() == o.tobytes(), (b.name, s, "per-scan chain")
            assert (dbits(tb[s]), dbits(te[s])) == (dbits(cb), dbits(ce)), (b.name, s)
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("lidar_type", [1, 2, 3])
def test_decode_scans_dev_on_every_batch_case(hip_lib, scene, lidar_type):
    g = hip_lib.LegKiloHip(scene.cfg())
    try:
        cases = [b for b in cc.BATCH_CASES if b.lidar_type == lidar_type]
        assert {b.name.split("[")[0].rstrip("0123456789").rstrip("_") for b in cases} >= {"collapsed_run", "equal_key_boundary", "all_cases_one_run",
                                                                                          "over_limit_run", "many_messages"}
        for k, b in enumerate(cases):
            if b.refused_message is None:
                _assert_run(g, b, seed=k)
                continue
            r = _Run(g, b, k)
            try:
                with pytest.raises(hip_lib.LegKiloError, match=rf"error -1: .*message {b.refused_message}: voxel grid leaf too small"):
                    r.batch()
                # every message but the refused one is a valid scan of the per-scan chain
                for s in (b.refused_message - 1, b.refused_message + 1):
                    dec = oracle_decode(b.msgs[s], b.lidar_type, b.time_scale, b.filter_num, b.blind, float(r.stamps[s]))[0]
                    assert_same_points(r.chain(s)[0], po.preprocess(dec, b.leaf), (b.name, s))
            finally:
                r.free()
            valid = next(x for x in cases if x.name.startswith("collapsed_run"))      # a valid run on the same handle
            _assert_run(g, valid, seed=99)
    finally:
        g.close()


@pytest.mark.gpu
def test_host_wrappers_equal_the_device_pointer_entries(hip_lib, scene):
    g = hip_lib.LegKiloHip(scene.cfg())
    try:
        for name in ("halves[1]", "halves[2]", "halves[3]"):
            c = cc.decode_case(name)
            dev, db, de = _decode_dev(g, c)
            got, tb, te = g.decode_scan(c.raw.tobytes(), len(c.raw), c.layout, c.time_scale, c.filter_num, c.blind, header_stamp=c.header_stamp)
            assert got.tobytes() == dev.tobytes() and len(got) > 10, name
            assert (dbits(tb), dbits(te)) == (dbits(db), dbits(de)), name
            assert_same_points(got, case_decode(c)[0], name)
        for name in ("faces_xyz[0.5]", "faces_xyz[0.3]", "stamps[0.5]", "stamps[0.3]"):
            c = cc.grid_case(name)
            got = g.preprocess_scan(c.pts, c.leaf)
            assert got.tobytes() == _preprocess_dev(g, c.pts, c.leaf).tobytes() and len(got) > 10, name
            assert_same_points(got, oracle_grid(name), name)
    finally:
        g.close()
