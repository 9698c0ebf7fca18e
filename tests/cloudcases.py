"""Crafted PointCloud2 messages and lk_point clouds that land WHERE THE LIDAR FRONT END DECIDES (tests/test_cloud_edges.py).

synth.vlp16_scan / dense_scan and the _spread / _collapsed clouds of tests/test_dev_bounds.py draw coordinates and time offsets from continuous
distributions; such values almost never meet the points at which lidar_processing.cc:25-108 and pcl::VoxelGrid (oracle/preprocess_oracle.py)
take one branch or the other.  Every case here is built by SEARCH over representable neighbours (np.nextafter, +-1 ns) and asserted, in this
module, to hit what it claims - an edited generator cannot silently stop producing the edge:

  decode   halves          (t - t_first) * 500 == k + 0.5 exactly in the handler's arithmetic, after AND before the first point, with the nearest
                           stamp on either side that gives another value                       (round half away from zero; the sign)
           minus_zero      offsets in (-1 ms, 0): round() gives -0.0, beside +0.0
           blind_edge      x*x + y*y + z*z (float32, unfused, left to right) == blind^2 (kept), one ulp under (dropped), one over; points where
                           the contracted sum fma(z, z, fma(x, x, y*y)) lies on the other side
           blind0          blind = 0 and a point at the origin (kept: 0 > 0 is false)
           filter_ge_n / filter_n_minus_1 / first_blind     filter_num >= n, filter_num == n - 1, point 0 inside the blind radius (times still come from it)
           ouster_large_t  t near 2^24, 2^31 and 2^32 - 1 ns, the first stamp the largest
           scaled          Velodyne stamps in microseconds, time_scale 1e-6
           odd_layout      a layout of our own: odd point_step, the time field ahead of x, no field 4-byte aligned
  grid     faces_x/y/z/xyz float32(k * leaf), k = -40 .. 40, with both neighbours; leaf 0.5 (1 / leaf exact) and 0.3 (inexact)
           zeros_*         +-0.0, +-1e-40, +-2^-149, +-1e-38 as coordinates and stamps: the minimum -0.0, a negative denormal, or -5
           under_limit / over_limit   1290^3 and 1291 * 1290^2 cells at leaf 0.5 (2^31 - 1 = 2 147 483 647 lies between)
           order_visible   cells of 3 .. 300 points whose float32 sums depend on the order
           stamps          negative stamps, stamps one ulp apart, 320 cells on one stamp, multi-point cells whose centroid stamp equals a
                           single-point cell's, a centroid stamp of -0.0 beside +0.0
  batch    collapsed_run, equal_key_boundary, many_messages, all_cases_one_run (a run has ONE layout, time_scale, filter_num, blind and leaf:
           per handler, one run per parameter set with the cases that share it - the grid cases travel as messages with blind 0 - and
           `_whole`, every message of the handler's own layout in one run under filter_num 1, blind 0, leaf 0.5), over_limit_run

Out of scope: NaN / infinite coordinates and |p / leaf| >= 2^31 (PCL's own int cast is undefined there).
"""
import collections
from fractions import Fraction

import numpy as np

import preprocess_oracle as po
from legkilo_amd import synth

F32 = np.float32
DTYPES = {1: po.VELODYNE_DTYPE, 2: po.OUSTER_DTYPE, 3: po.HESAI_DTYPE}
TNAME = synth.CLOUD_TIME_FIELD
SCALE = synth.CLOUD_TIME_SCALE
LEAVES = (0.5, 0.3)
BLIND = 1.5
STAMP = 1234.5        # header stamp of the single-message cases
EPOCH = 1.7e9
# the same fields in an order and at offsets of our own: odd point_step, time first, no field on a 4-byte boundary
ODD_DTYPES = {
    1: np.dtype({"names": ["time", "x", "y", "z"], "formats": ["<f4", "<f4", "<f4", "<f4"], "offsets": [1, 6, 11, 17], "itemsize": 23}),
    2: np.dtype({"names": ["t", "x", "y", "z"], "formats": ["<u4", "<f4", "<f4", "<f4"], "offsets": [1, 6, 11, 17], "itemsize": 23}),
    3: np.dtype({"names": ["timestamp", "x", "y", "z"], "formats": ["<f8", "<f4", "<f4", "<f4"], "offsets": [1, 10, 15, 21], "itemsize": 27}),
}

DecodeCase = collections.namedtuple("DecodeCase", "name lidar_type raw layout time_scale filter_num blind header_stamp")
GridCase = collections.namedtuple("GridCase", "name pts leaf refused")
BatchCase = collections.namedtuple("BatchCase", "name lidar_type msgs layout time_scale filter_num blind leaf refused_message")


# ----------------------------------------------------------------------------------------------------------------- representable neighbours
def neighbours(x, w):
    """x and its w representable neighbours on either side, ascending along axis 0 (float arrays: np.nextafter; integer arrays: +-1)."""
    x = np.asarray(x)
    if x.dtype.kind in "iu":
        return np.stack([x.astype(np.int64) + d for d in range(-w, w + 1)])
    lo, hi = [x], [x]
    for _ in range(w):
        lo.append(np.nextafter(lo[-1], x.dtype.type(-np.inf)))
        hi.append(np.nextafter(hi[-1], x.dtype.type(np.inf)))
    return np.stack(lo[:0:-1] + hi)


def round_f32(q):
    """The float32 nearest to the rational q, ties to even - one rounding, whatever q's width."""
    r = F32(float(q))
    best = None
    for c in (np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf))):
        key = (abs(Fraction(float(c)) - q), int(c.view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def fma32(a, b, c):
    """fmaf(a, b, c): the exact a * b + c, rounded once."""
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ----------------------------------------------------------------------------------------------------------------- the handlers' arithmetic
def scaled_offset(lidar_type, time_scale, raw_t, raw_first):
    """(t - t_first) * 500 as the handler forms it (lidar_processing.cc:47-48, :75-76, :103-104): the value std::round is given.  Velodyne and
    Ouster: time_scale * t rounded to float, float difference, float product; Hesai: doubles throughout."""
    t = np.asarray(raw_t).astype(np.float64)
    if lidar_type == 3:
        return (np.float64(time_scale) * t - np.float64(time_scale) * np.float64(raw_first)) * np.float64(500.0)
    first = F32(np.float64(time_scale) * np.float64(raw_first))
    cur = (np.float64(time_scale) * t).astype(F32)
    return ((cur - first).astype(F32) * F32(500.0)).astype(F32)


def _raw_time(lidar_type, seconds, time_scale):
    """The raw stamp nearest to `seconds` (float64) in the handler's field type."""
    v = np.asarray(seconds, dtype=np.float64) / time_scale
    return {1: lambda: v.astype(F32), 2: lambda: np.round(v).astype(np.int64), 3: lambda: v}[lidar_type]()


def half_stamps(lidar_type, time_scale, raw_first, sign, ks, w):
    """For every k of ks: the raw stamps within w neighbours of t_first + sign * (k + 0.5) / 500 whose scaled offset is exactly sign * (k + 0.5) -
    the first and last of that run of stamps - and the nearest stamp on either side of the run, whose offset differs.  -> (stamps, number of
    k with an exact half)."""
    first_s = float(np.float64(time_scale) * np.float64(raw_first))
    out, hits = [], 0
    for k in ks:
        want = sign * (k + 0.5)
        win = neighbours(_raw_time(lidar_type, first_s + want / 500.0, time_scale), w)
        if lidar_type == 2:
            win = win[(win >= 0) & (win < 2 ** 32)]
        hit = np.flatnonzero(scaled_offset(lidar_type, time_scale, win, raw_first) == want)
        if hit.size == 0:
            continue
        mid = hit[np.argmin(np.abs(hit - len(win) // 2))]
        a = b = mid
        while a - 1 in hit:
            a -= 1
        while b + 1 in hit:
            b += 1
        if a == 0 or b == len(win) - 1:
            continue          # the run leaves the window: no neighbour on that side
        hits += 1
        out += [win[a - 1], win[a], win[b], win[b + 1]]
    return out, hits


def _message(lidar_type, xyz, raw_t, dtype=None, seed=0):
    """A packed message: the handler's point layout (or `dtype`), the bytes of every field the decoder does not read random."""
    dt = DTYPES[lidar_type] if dtype is None else dtype
    n = len(raw_t)
    rng = np.random.default_rng([77, lidar_type, seed, n])
    raw = np.frombuffer(rng.integers(0, 256, size=n * dt.itemsize, dtype=np.uint8).tobytes(), dtype=dt).copy()
    xyz = np.asarray(xyz, dtype=F32).reshape(n, 3)
    raw["x"], raw["y"], raw["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    raw[TNAME[lidar_type]] = np.asarray(raw_t).astype(dt.fields[TNAME[lidar_type]][0])
    return raw


def _layout(lidar_type, dtype=None):
    return synth.cloud_layout(lidar_type, dtype)


def _line(n, x0=2.0, step=0.07):
    """n points outside the blind radius, a few per 0.3 / 0.5 m cell."""
    i = np.arange(n)
    return np.stack([x0 + step * i, 1.0 + 0.11 * (i % 5), 0.5 - 0.13 * (i % 3)], axis=1).astype(F32)


def _decode_case(name, lidar_type, xyz, raw_t, time_scale=None, filter_num=1, blind=BLIND, dtype=None, seed=0):
    raw = _message(lidar_type, xyz, raw_t, dtype, seed)
    return DecodeCase(f"{name}[{lidar_type}]", lidar_type, raw, _layout(lidar_type, dtype), SCALE[lidar_type] if time_scale is None else time_scale,
                      filter_num, blind, STAMP)


# ----------------------------------------------------------------------------------------------------------------- decode cases
HALVES = {}     # (lidar_type, first) -> (exact halves after, exact halves before the first point)


def _halves_case(name, lidar_type, raw_first, ks, w, time_scale=None, dtype=None):
    ts = SCALE[lidar_type] if time_scale is None else time_scale
    after, na = half_stamps(lidar_type, ts, raw_first, +1, ks, w)
    before, nb = half_stamps(lidar_type, ts, raw_first, -1, ks, w)
    HALVES[(name, lidar_type)] = (na, nb)
    t = [raw_first] + [v for pair in zip(after, before) for v in pair] + after[len(before):] + before[len(after):]   # signs interleaved
    return _decode_case(name, lidar_type, _line(len(t)), t, time_scale=time_scale, dtype=dtype)


def _minus_zero_case(lidar_type):
    ts = SCALE[lidar_type]
    first_s = {1: 0.05, 2: 0.05, 3: EPOCH}[lidar_type]
    raw_first = _raw_time(lidar_type, first_s, ts)
    off = np.array([-0.0009, -0.0005, -0.0001, -0.00003, 0.0, 0.00003, 0.0004, 0.0009, -0.00099, 0.00099])
    t = np.r_[raw_first, _raw_time(lidar_type, float(np.float64(ts) * np.float64(raw_first)) + off, ts)]
    v = scaled_offset(lidar_type, ts, t, t[0])
    assert np.sum((v < 0) & (v > -0.5)) >= 4 and np.sum((v >= 0) & (v < 0.5)) >= 4, v      # -0.0 and +0.0 after std::round
    return _decode_case("minus_zero", lidar_type, _line(len(t)), t)


def sumsq(x, y, z):
    """x*x + y*y + z*z in float32, every product and sum rounded, left to right (blindCheck, lidar_processing.h:96-98)."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    return ((x * x).astype(F32) + (y * y).astype(F32)).astype(F32) + (z * z).astype(F32)


def sumsq_fused(x, y, z):
    """The same expression as a compiler contracts it: fma(z, z, fma(x, x, y*y)) (scalars; exact)."""
    return fma32(z, z, fma32(x, x, F32(F32(y) * F32(y))))


def _blind_points(blind, want=12):
    """Points on the blind sphere in float32: sum == blind^2, one ulp under, one ulp over, and points whose contracted sum lies on the other
    side of blind^2 than the plain one."""
    b2 = F32(blind) * F32(blind)
    under, over = np.nextafter(b2, F32(0)), np.nextafter(b2, F32(np.inf))
    rng = np.random.default_rng(1501)
    got = {"eq": [], "under": [], "over": [], "straddle": []}
    while min(len(v) for v in got.values()) < want:
        x, y = (rng.uniform(-0.6, 0.6, 2) * blind).astype(F32)
        z0 = np.sqrt(b2 - x * x - y * y).astype(F32) * F32(rng.choice([-1.0, 1.0]))
        for z in neighbours(z0, 6):
            s = sumsq(x, y, z)
            kind = "eq" if s == b2 else "under" if s == under else "over" if s == over else None
            if kind and len(got[kind]) < want:
                got[kind].append((x, y, z))
            if abs(float(s) - float(b2)) < 1e-6 and len(got["straddle"]) < want and (s >= b2) != (sumsq_fused(x, y, z) >= b2):
                got["straddle"].append((x, y, z))
    return {k: np.array(v, dtype=F32) for k, v in got.items()}, b2


BLIND_POINTS, BLIND2 = _blind_points(BLIND)


def _blind_edge_case(lidar_type):
    p = BLIND_POINTS
    xyz = np.concatenate([_line(1), p["eq"], p["under"], p["over"], p["straddle"]])
    order = np.r_[0, 1 + np.random.default_rng(3).permutation(len(xyz) - 1)]
    t = _raw_time(lidar_type, (EPOCH if lidar_type == 3 else 0.0) + 0.002 * (np.arange(len(xyz)) % 50), SCALE[lidar_type])
    return _decode_case("blind_edge", lidar_type, xyz[order], t)


def _blind0_case(lidar_type):
    xyz = np.array([[0, 0, 0], [-0.0, 0.0, -0.0], [1e-30, 0, 0], [0.4, -0.3, 0.2], [2, 1, 0.5]], dtype=F32)
    t = _raw_time(lidar_type, (EPOCH if lidar_type == 3 else 0.0) + 0.003 * np.arange(len(xyz)), SCALE[lidar_type])
    return _decode_case("blind0", lidar_type, xyz, t, blind=0.0)


def _filter_cases(lidar_type):
    n = 7
    t = _raw_time(lidar_type, (EPOCH if lidar_type == 3 else 0.0) + 0.0031 * np.arange(n), SCALE[lidar_type])
    inside = _line(n)
    inside[0] = (0.3, 0.2, 0.1)          # point 0 inside the blind radius: dropped, but begin / end and every offset still come from it
    return [_decode_case("filter_ge_n", lidar_type, _line(n), t, filter_num=n),
            _decode_case("filter_n_minus_1", lidar_type, _line(n), t, filter_num=n - 1),
            _decode_case("first_blind", lidar_type, inside, t[::-1].copy())]


def _ouster_large_t_case():
    t = [2 ** 32 - 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 129, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 129, 2 ** 32 - 2,
         2 ** 32 - 257, 5, 0, 2 ** 31 + 1_000_000, 2 ** 24 + 1_000_000]
    f = (np.float64(1e-9) * np.array(t, dtype=np.float64)).astype(F32)
    assert f[0] == f.max() and len(np.unique(f)) < len(t)          # the first stamp is the largest; neighbouring ns collapse onto one float
    return _decode_case("ouster_large_t", 2, _line(len(t)), t)


def _repack(case, name, dtype):
    raw = case.raw
    lt = case.lidar_type
    xyz = np.stack([raw["x"], raw["y"], raw["z"]], axis=1)
    return _decode_case(name, lt, xyz, raw[TNAME[lt]], time_scale=case.time_scale, filter_num=case.filter_num, blind=case.blind, dtype=dtype, seed=9)


def _decode_cases():
    cases = []
    for lt in (1, 2, 3):
        ts = SCALE[lt]
        if lt == 3:
            h = [_halves_case("halves", 3, EPOCH, (62, 187), 3), _halves_case("halves_first_0.25", 3, 0.25, range(120), 3)]
            assert HALVES[("halves", 3)] == (2, 2)                       # +-0.125 s and +-0.375 s: the only exact halves at a 2^-22 s granularity
            assert min(HALVES[("halves_first_0.25", 3)]) >= 20, HALVES
        else:
            first = {1: (0.0, 0.1), 2: (0, 120_000_000)}[lt]
            h = [_halves_case("halves", lt, _raw_time(lt, first[0] * ts, ts) if lt == 1 else first[0], range(60), 64 if lt == 2 else 3),
                 _halves_case("halves_late_first", lt, F32(first[1]) if lt == 1 else first[1], range(60), 64 if lt == 2 else 3)]
            na = sum(HALVES[(c, lt)][0] for c in ("halves", "halves_late_first"))
            nb = sum(HALVES[(c, lt)][1] for c in ("halves", "halves_late_first"))
            assert na >= 20 and nb >= 20, HALVES
        cases += h
        cases.append(_minus_zero_case(lt))
        cases.append(_blind_edge_case(lt))
        cases.append(_blind0_case(lt))
        cases += _filter_cases(lt)
        if lt == 2:
            cases.append(_ouster_large_t_case())
        if lt == 1:
            cases.append(_halves_case("scaled", 1, F32(0.0), range(60), 3, time_scale=1e-6))
            assert min(HALVES[("scaled", 1)]) >= 20, HALVES
        cases.append(_repack(h[0], "odd_layout", ODD_DTYPES[lt]))
    return cases


# ----------------------------------------------------------------------------------------------------------------- grid cases
def cell_of(v, leaf):
    """floor(v * (1 / leaf)) in float32, as PCL forms it (voxel_grid.hpp), per coordinate -> int64."""
    inv = F32(1.0) / F32(leaf)
    return np.floor((np.asarray(v, dtype=F32) * inv).astype(F32)).astype(np.int64)


def _points(xyz, curv):
    xyz = np.asarray(xyz, dtype=F32).reshape(-1, 3)
    pts = np.zeros(len(xyz), dtype=synth.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["curvature"] = np.asarray(curv, dtype=F32)
    return pts


def _face_values(leaf):
    ks = np.arange(-40, 41)
    face = (ks * leaf).astype(F32)
    vals = neighbours(face, 1)                       # (3, 81): below, on, above
    c = cell_of(vals, leaf)
    if leaf == 0.5:
        assert np.array_equal(c[1], ks) and np.array_equal(c[0], ks - 1) and np.array_equal(c[2], ks)
    else:                                            # 1 / 0.3 is inexact: float32(k * 0.3) * inv falls on either side of k
        assert np.sum(c[1] == ks) >= 10 and np.sum(c[1] == ks - 1) >= 10, (np.sum(c[1] == ks), np.sum(c[1] == ks - 1))
    return vals.T.reshape(-1)                        # 243 values, ascending


def _faces_cases(leaf):
    v = _face_values(leaf)
    n = len(v)
    i = np.arange(n)
    curv = (F32(0.002) * ((i * 37) % 50).astype(F32)).astype(F32)
    rest = F32(0.1)
    out = []
    for a, ax in enumerate("xyz"):
        xyz = np.full((n, 3), rest, dtype=F32)
        xyz[:, a] = v[(i * 5 + a) % n]               # not in ascending order
        out.append(GridCase(f"faces_{ax}[{leaf}]", _points(xyz, curv), leaf, False))
    xyz = np.stack([v, v[(i * 7 + 3) % n], v[(i * 11 + 5) % n]], axis=1)
    out.append(GridCase(f"faces_xyz[{leaf}]", _points(xyz, curv), leaf, False))
    return out


SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), 1e-38, -1e-38]).astype(F32)
assert np.all(np.abs(SPECIALS[2:]) < np.finfo(F32).tiny) and np.all(SPECIALS[2:] != 0)    # denormals, not flushed by the cast


def _zeros_cases(leaf):
    def cloud(vals, extra):
        g = np.array([(a, b, c) for a in vals for b in vals for c in vals], dtype=F32)
        g = g[np.random.default_rng(len(vals)).permutation(len(g))]
        far = np.array([[0.7, 0.2, 0.9], [1.3, 0.1, 0.05], [0.2, 2.2, 0.3]], dtype=F32)
        xyz = np.concatenate([g[:5], far, extra, g[5:]]).astype(F32)
        curv = np.r_[SPECIALS, F32(0.002), F32(-0.002), F32(1.0)][np.arange(len(xyz)) * 3 % 11]
        if len(extra):
            curv[[5, 8]] = 0.5       # far[0] and the extra point, each alone in its cell, on one stamp: the tie shows their CELL order, which min_b decides
        return _points(xyz, curv)

    none = np.zeros((0, 3), dtype=F32)
    full = cloud(SPECIALS, none)
    nonneg = cloud(SPECIALS[[0, 1, 2, 4, 6]], none)
    m5 = cloud(SPECIALS, np.array([[-5, -5, -5]], dtype=F32))
    # a negative denormal has a cell of its own: -1, not 0 (what flushing it to zero would give)
    assert np.all(cell_of(SPECIALS[[3, 5, 7]], leaf) == -1) and np.all(cell_of(SPECIALS[[0, 1, 2, 4, 6]], leaf) == 0)
    ids = [tuple(int(cell_of(m5[f][i], leaf)) for f in "xyz") for i in range(len(m5))]
    assert ids.count(ids[5]) == 1 and ids.count(ids[8]) == 1 and m5["x"][8] == -5 and m5["curvature"][5] == m5["curvature"][8]
    assert full["x"].min() == SPECIALS[7] and m5["x"].min() == -5 and cell_of(nonneg["x"], leaf).min() == 0 and np.signbit(nonneg["x"]).any()
    return [GridCase(f"zeros_min_denormal[{leaf}]", full, leaf, False), GridCase(f"zeros_min_negzero[{leaf}]", nonneg, leaf, False),
            GridCase(f"zeros_min_m5[{leaf}]", m5, leaf, False)]


def _limit_case(nx, name, refused):
    """nx x 1290 x 1290 cells at leaf 0.5: the two corners and 200 interior points, all on multiples of 0.25 (exact)."""
    rng = np.random.default_rng(nx)
    ext = np.array([nx, 1290, 1290])
    cells = np.concatenate([[[0, 0, 0]], rng.integers(0, ext, size=(200, 3)), [ext - 1], rng.integers(0, ext, size=(8, 3))])
    cells[5] = cells[40]                                        # two points of one cell
    xyz = (cells * 0.5 + 0.25 * rng.integers(0, 2, size=cells.shape)).astype(F32)
    xyz[[0, 201]] = (cells[[0, 201]] * 0.5).astype(F32)         # the corners exactly on their cells' lower faces
    pts = _points(xyz, (F32(0.002) * (np.arange(len(xyz)) % 50).astype(F32)).astype(F32))
    c = np.stack([cell_of(pts[f], 0.5) for f in "xyz"], axis=1)
    div = c.max(0) - c.min(0) + 1
    assert np.array_equal(div, ext) and np.array_equal(c.min(0), [0, 0, 0])
    key = c[:, 0] + c[:, 1] * int(div[0]) + c[:, 2] * int(div[0]) * int(div[1])
    assert (int(div[0]) * int(div[1]) * int(div[2]) > 2 ** 31 - 1) == refused
    if not refused:
        assert int(key.max()) == 2_146_688_999 == 1290 ** 3 - 1
    return GridCase(name, pts, 0.5, refused)


def cell_sum(v, order):
    """float32 sum of one cell's values: "seq" (input order, the definition), "reverse", "pairwise" (halves, recursively)."""
    v = [F32(a) for a in v]
    if order == "pairwise":
        if len(v) <= 2:
            return F32(v[0] + v[1]) if len(v) == 2 else v[0]
        h = len(v) // 2
        return F32(cell_sum(v[:h], order) + cell_sum(v[h:], order))
    acc = F32(0)
    for a in (v[::-1] if order == "reverse" else v):
        acc = F32(acc + a)
    return acc


ORDER_SIZES = (3, 4, 5, 7, 16, 33, 64, 150, 257, 300)
ORDER_VISIBLE = {}     # leaf -> (cells whose centroid changes under "reverse", under "pairwise")


def _order_visible_case(leaf):
    rng = np.random.default_rng(int(leaf * 10))
    xyz, curv, cell = [], [], []
    for c, m in enumerate(ORDER_SIZES + ORDER_SIZES):
        base = np.array([(c % 5) - 2, (c // 5) - 1, c % 3], dtype=np.float64) * leaf
        xyz.append(base + rng.uniform(0.02, leaf - 0.02, size=(m, 3)))
        big = np.tile([1.0e8, 1.0, -1.0e8], m // 3 + 1)[:m] * (1 + 0.25 * rng.integers(0, 3, m)) if c < len(ORDER_SIZES) else rng.uniform(0, 0.1, m)
        curv.append(big)
        cell += [c] * m
    xyz, curv, cell = np.concatenate(xyz).astype(F32), np.concatenate(curv).astype(F32), np.array(cell)
    perm = np.random.default_rng(8).permutation(len(cell))      # the cells' points interleaved in the input
    pts, cell = _points(xyz[perm], curv[perm]), cell[perm]
    ids = np.stack([cell_of(pts[f], leaf) for f in "xyz"], axis=1)
    assert len({tuple(r) for r in ids}) == len(ORDER_SIZES) * 2 and all(len({tuple(r) for r in ids[cell == c]}) == 1 for c in range(cell.max() + 1))
    vis = {"reverse": 0, "pairwise": 0}
    for c in range(cell.max() + 1):
        m = cell == c
        for order in vis:
            if any(cell_sum(pts[f][m], order).tobytes() != cell_sum(pts[f][m], "seq").tobytes() for f in pts.dtype.names):
                vis[order] += 1
    ORDER_VISIBLE[leaf] = (vis["reverse"], vis["pairwise"])
    assert min(vis.values()) >= 10, vis
    return GridCase(f"order_visible[{leaf}]", pts, leaf, False)


TIE_RUN = 320


def _stamps_case(leaf):
    """One cell per lattice site (the point at the cell's centre; the sites taken in an order of our own, so cell order != input order)."""
    sites = [(i, j, k) for k in range(2) for j in range(24) for i in range(24) if (i, j, k) not in ((3, 0, 0), (5, 0, 0))]
    take = iter(np.random.default_rng(11).permutation(len(sites)))
    xyz, curv = [], []

    def cell(stamps, site=None):
        s = np.array(sites[next(take)] if site is None else site, dtype=np.float64)
        for q, t in enumerate(stamps):
            xyz.append((s + 0.5 + 0.1 * (q % 3 - 1) * (q > 0)) * leaf)
            curv.append(t)

    for t in (-0.3, -0.002, -1e-40, -(2.0 ** -149), -1e-38, 2.0 ** -149, 1e-40, 0.0):
        cell([t])
    for t in (-0.1, -0.002, -1e-38, 0.05, 1.0, 0.002):         # stamps one ulp apart, in single-point cells
        for v in neighbours(F32(t), 1):
            cell([v])
    for _ in range(TIE_RUN):
        cell([0.05])
    for _ in range(3):                                         # centroid stamps equal to single-point cells' stamps, on either side in cell order
        cell([0.5]), cell([0.25, 0.75]), cell([2.0]), cell([1.0, 2.0, 3.0]), cell([0.05]), cell([0.025, 0.075])
    # a centroid stamp of -0.0 (-2^-149 / 2 rounds to it) in the LAST cell, +0.0 in cells before it: equal keys of the time sort, cell order decides
    cell([0.0], site=(3, 0, 0)), cell([-0.0, 0.0], site=(5, 0, 0)), cell([-(2.0 ** -149), 0.0], site=(23, 23, 2)), cell([0.0, 0.0], site=(22, 23, 2))
    perm = np.random.default_rng(12).permutation(len(curv))
    pts = _points(np.array(xyz)[perm], np.array(curv)[perm])
    ids = np.stack([cell_of(pts[f], leaf) for f in "xyz"], axis=1)
    assert len({tuple(r) for r in ids}) == 8 + 18 + TIE_RUN + 18 + 4
    assert np.sum(pts["curvature"] == F32(0.05)) >= TIE_RUN and np.sum(pts["curvature"] < 0) >= 10
    assert (F32(-(2.0 ** -149)) / F32(2)).tobytes() == F32(-0.0).tobytes()
    return GridCase(f"stamps[{leaf}]", pts, leaf, False)


def _grid_cases():
    out = []
    for leaf in LEAVES:
        out += _faces_cases(leaf) + _zeros_cases(leaf) + [_order_visible_case(leaf), _stamps_case(leaf)]
    out.append(_limit_case(1290, "under_limit", False))
    out.append(_limit_case(1291, "over_limit", True))
    return out


# ----------------------------------------------------------------------------------------------------------------- batch cases
def as_message(pts, lidar_type, seed=0):
    """An lk_point cloud as a message of the handler: its xyz, and stamps on the 2 ms bins (bin = point index mod 50)."""
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1)
    t = _raw_time(lidar_type, (EPOCH if lidar_type == 3 else 0.0) + 0.002 * (np.arange(len(pts)) % 50), SCALE[lidar_type])
    return _message(lidar_type, xyz, t, seed=seed)


def _batch(name, lidar_type, clouds, leaf, refused_message=None):
    msgs = [as_message(c, lidar_type, seed=s) for s, c in enumerate(clouds)]
    return BatchCase(f"{name}[{lidar_type}]", lidar_type, msgs, _layout(lidar_type), SCALE[lidar_type], 1, 0.0, leaf, refused_message)


def _one_cell(n, seed, leaf=0.5, cell=(0, 0, 0)):
    rng = np.random.default_rng(seed)
    return _points((np.array(cell) + rng.uniform(0.1, 0.9, size=(n, 3))) * leaf, np.zeros(n))


def sorted_keys(pts, leaf):
    """The scan's cell keys, ascending (ijk relative to the scan's own minimum, x fastest)."""
    c = np.stack([cell_of(pts[f], leaf) for f in "xyz"], axis=1)
    c -= c.min(0)
    d = c.max(0) + 1
    return np.sort(c[:, 0] + c[:, 1] * d[0] + c[:, 2] * d[0] * d[1])


def _collapsed_run(lidar_type):
    clouds = [_one_cell(3 + 5 * s, 100 + s) for s in range(12)]
    assert all(np.all(sorted_keys(c, 0.5) == 0) for c in clouds)
    return _batch("collapsed_run", lidar_type, clouds, 0.5)


def _equal_key_boundary(lidar_type):
    kinds = {"A": [(0, 0, 0), (1, 0, 0)], "B": [(1, 0, 0), (0, 1, 0)], "C": [(0, 1, 0), (1, 0, 1)]}      # keys {0, 1}, {1, 2}, {2, 5}
    clouds = []
    for s, kind in enumerate("ABCABCAB"):
        parts = [_one_cell(2 + (s + q) % 3, 200 + 10 * s + q, cell=c) for q, c in enumerate(kinds[kind])]
        clouds.append(np.concatenate(parts)[::-1].copy())
    keys = [sorted_keys(c, 0.5) for c in clouds]
    same = [s for s in range(len(keys) - 1) if keys[s][-1] == keys[s + 1][0] != 0]
    assert len(same) >= 5, same
    return _batch("equal_key_boundary", lidar_type, clouds, 0.5)


def _many_messages(S, lidar_type):
    rng = np.random.default_rng(S)
    clouds = [_points(rng.uniform(-3, 3, size=(1 + s % 3, 3)), np.zeros(1 + s % 3)) for s in range(S)]
    return _batch(f"many_messages_{S}", lidar_type, clouds, 0.3)


def _case_runs(lidar_type):
    """Every decode case of the handler and every grid case that is not refused, as messages of runs: one run per (layout, time_scale,
    filter_num, blind, leaf).  The decode cases keep their own parameters and run at both leaves; the grid cases are messages under blind 0,
    filter_num 1 at their own leaf, together with the blind-0 decode case."""
    runs = collections.OrderedDict()
    for leaf in LEAVES:
        for c in DECODE_CASES:
            if c.lidar_type == lidar_type:
                key = (tuple(sorted(c.layout.items())), c.time_scale, c.filter_num, c.blind, leaf)
                runs.setdefault(key, []).append(c.raw)
        key = (tuple(sorted(_layout(lidar_type).items())), SCALE[lidar_type], 1, 0.0, leaf)
        for k, g in enumerate(GRID_CASES):
            if g.leaf == leaf and not g.refused:
                runs.setdefault(key, []).append(as_message(g.pts, lidar_type, seed=k))
    out = []
    for r, ((lay, ts, fn, blind, leaf), msgs) in enumerate(runs.items()):
        out.append(BatchCase(f"all_cases_one_run_{r}[{lidar_type}]", lidar_type, msgs, dict(lay), ts, fn, blind, leaf, None))
    assert sum(len(b.msgs) for b in out) == 2 * sum(c.lidar_type == lidar_type for c in DECODE_CASES) + sum(not g.refused for g in GRID_CASES)
    # and literally ONE run: every message in the handler's own layout, whatever its case's parameters, under filter_num 1, blind 0, leaf 0.5
    std = _layout(lidar_type)
    msgs = [c.raw for c in DECODE_CASES if c.lidar_type == lidar_type and c.layout == std]
    msgs += [as_message(g.pts, lidar_type, seed=k) for k, g in enumerate(GRID_CASES) if not g.refused]
    assert len(msgs) == sum(c.lidar_type == lidar_type for c in DECODE_CASES) - 1 + len(GRID_CASES) - 1      # all but odd_layout and over_limit
    out.append(BatchCase(f"all_cases_one_run_whole[{lidar_type}]", lidar_type, msgs, std, SCALE[lidar_type], 1, 0.0, 0.5, None))
    return out


def _over_limit_run(lidar_type):
    clouds = [_one_cell(4 + s, 300 + s) for s in range(8)]
    clouds[5] = next(g.pts for g in GRID_CASES if g.name == "over_limit")
    clouds[6] = next(g.pts for g in GRID_CASES if g.name == "under_limit")
    return _batch("over_limit_run", lidar_type, clouds, 0.5, refused_message=5)


def _batch_cases():
    out = []
    for lt in (1, 2, 3):
        out += [_collapsed_run(lt), _equal_key_boundary(lt), _over_limit_run(lt)] + _case_runs(lt)
    out += [_many_messages(S, lt) for S, lt in ((1, 3), (255, 1), (256, 2), (257, 1))]
    return out


DECODE_CASES = _decode_cases()
GRID_CASES = _grid_cases()
BATCH_CASES = _batch_cases()
for _cases in (DECODE_CASES, GRID_CASES, BATCH_CASES):
    assert len({c.name for c in _cases}) == len(_cases)


def decode_case(name):
    return next(c for c in DECODE_CASES if c.name == name)


def grid_case(name):
    return next(c for c in GRID_CASES if c.name == name)


def run_stamps(n, t0=100.0):
    """Header stamps of a run's messages: ascending, 0.1 s apart."""
    return t0 + 0.1 * np.arange(n)
