"""The frozen table of plane-extraction cases (lk_clouds_planes_dev, lk_clouds_planes): seeded, listed by name, small.

A case is a dict: cloud [n, 3] (float32), dist, n_hyp, max_planes, min_inliers, axis (None or three floats), cos_max_angle, seed, flags.  build() is
the seeded generator; the table the tests use (CASES) is its output as FROZEN in tests/golden/planecloud_cases.npz, beside each case's expected
values: the label and keep flag per point, per plane n_inliers and hyp, the counts and the status - all from EXACT rational arithmetic on the float
coordinates - and per plane normal, d, centroid, eig and rmse from 50-digit arithmetic.  tests/golden/make_planecloud_cases.py writes the file and
ASSERTS that every decision of the table is clear:
  * membership s*s <= t2q by a relative 2^-40 (the float64 evaluation makes about ten roundings of 2^-53), or an exact tie;
  * the axis test g*g < c2 q aa by the same margin, or an exact tie;
  * the winner ahead of the runner-up by at least one inlier, or a tie of scores (the smallest h is taken).
So labels, counts, hyp, offsets, kept records and src_idx are whole numbers and are compared exactly, no case left out.  THRESHOLD_TIES names the
cases in which some s*s equals t2q exactly, SCORE_TIES those in which a round's best score is reached by several hypotheses; the generator asserts
that these lists are the ones it finds.  The coefficients are compared under err <= C * 2^-53 * scale (C_NORMAL with scale 1 for the normal, C_COORD
with the largest |coordinate| of the cloud for centroid and d and its square for eig and rmse^2): C is 16 times what the float64 numpy statement
itself reaches on the table, the figures below, the rule of tests/test_filter_solvers.py.  A refit whose two smallest eigenvalues lie within
GAP_FRACTION of the largest (the generator decides at 50 digits) has no conditioned normal: only its eig and centroid are compared.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planecloud_cases.npz")

GROUP, TILE, CHUNK = 64, 256, 2048   # lk_planes.h's LK_PLANES_GROUP / _TILE / _CHUNK (tests/test_planes_host.py holds them against the header)
DIST = 0.015625                      # the parameters of most cases, so that they go into one call as many clouds
N_HYP = 64
MAX_PLANES = 3
MIN_INLIERS = 16
SEED = 20261021
KEEP_PLANES = 1
NONE = 0xFFFFFFFF
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1]
HYPS = [1, GROUP - 1, GROUP, GROUP + 1, 256]
PLACE = (3000.0, 2000.0, 100.0)
PARAMS = ("dist", "n_hyp", "max_planes", "min_inliers", "axis", "cos_max_angle", "seed", "flags")
THRESHOLD_TIES = ["thr_at", "thr_norm"]
SCORE_TIES = ["s256", "s3", "s4", "range_below", "h256", "coplanar", "two_planes_equal", "on_line_plus", "floor_wall", "floor_wall_free", "floor_wall_cos0", "tilt_free", "peel",
              "peel_max2", "peel_min201", "peel_keep_planes", "short_after_round"]
AXIS_TIES = ["floor_wall_cos0"]     # g*g == c2 q aa exactly: 0 == 0 for a wall under cos_max_angle 0 (not below: accepted)
GAP_FRACTION = 2.0 ** -20
# what the float64 numpy statement (cloudmetrics.planes) reaches on the table, in units of 2^-53 * scale, and 16 times that rounded up
NUMPY_REACHES_NORMAL, NUMPY_REACHES_COORD = 7.0, 2.008   # (on_line_plus; twin_a)
C_NORMAL, C_COORD = 112.0, 33.0
COS10 = float(np.cos(np.deg2rad(10.0)))


def case(cloud, dist=DIST, n_hyp=N_HYP, max_planes=MAX_PLANES, min_inliers=MIN_INLIERS, axis=None, cos_max_angle=0.0, seed=SEED, flags=0):
    return dict(cloud=np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 3)), dist=float(dist), n_hyp=int(n_hyp), max_planes=int(max_planes),
                min_inliers=int(min_inliers), axis=None if axis is None else tuple(float(v) for v in axis), cos_max_angle=float(cos_max_angle), seed=int(seed),
                flags=int(flags))


def q12(v):
    """coordinates as multiples of 2^-12: exact in float32 up to 2^12, and small integers for the exact evaluation"""
    return np.round(np.asarray(v, dtype=np.float64) * 4096.0) / 4096.0


def sample(seed, r, h, m):
    """lk_planes_sample in Python integers -> (i0, i1, i2)"""
    M = (1 << 64) - 1

    def mix(x):
        z = (x + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    ctr = (r * 4096 + h) * 4
    i0 = (mix((seed + ctr) & M) * m) >> 64
    i1 = (mix((seed + ctr + 1) & M) * (m - 1)) >> 64
    i2 = (mix((seed + ctr + 2) & M) * (m - 2)) >> 64
    i1 += i1 >= i0
    lo, hi = min(i0, i1), max(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return i0, i1, i2


def seed_where(ok, start=1):
    """the first seed from `start` on that ok(seed) accepts"""
    s = start
    while not ok(s):
        s += 1
    return s


def build():
    rng = np.random.default_rng(20261021)

    def planar(n, share=0.7, noise=0.03, side=4.0):
        """a noisy plane z = 0.1 x + 0.2 y through a box of scattered points, shuffled"""
        k = int(round(share * n))
        xy = rng.uniform(-side / 2, side / 2, size=(k, 2))
        on = np.c_[xy, 0.1 * xy[:, 0] + 0.2 * xy[:, 1] + rng.uniform(-noise, noise, size=k)]
        off = rng.uniform(-side / 2, side / 2, size=(n - k, 3))
        return q12(np.r_[on, off][rng.permutation(n)])

    cs = {}
    # ---- sizes: nothing, a point, a pair (no round runs), a wave, the score kernel's LDS tile and its record chunk with their neighbours.  The
    # invalid clouds and the empty one stand in the middle of the call
    for n in SIZES[:7]:
        if n not in (3, 4):
            cs[f"s{n}"] = case(planar(n))
    good = planar(60)
    for name, value in (("nan_cloud", np.nan), ("inf_cloud", -np.inf)):
        c = good.copy()
        c[11, 1] = value
        cs[name] = case(c)
    cs["empty_mid"] = case(np.zeros((0, 3)))
    for n in SIZES[7:]:
        cs[f"s{n}"] = case(planar(n))
    # ---- independence of the call: two clouds of one call with identical coordinates
    twin = planar(300)
    cs["twin_a"] = case(twin)
    cs["twin_b"] = case(twin)
    # ---- placement: the same cloud at the origin and at (3000, 2000, 100); every coordinate a multiple of 2^-12 below 2^12, so the sums are exact
    pl = planar(300)
    cs["place_origin"] = case(pl)
    cs["place_far"] = case(pl + np.array(PLACE))
    # ---- three and four points, and the range bound, at min_inliers 3: every hypothesis draws the same plane (score ties)
    small = dict(min_inliers=3)
    cs["s3"] = case([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.25]], **small)
    cs["s4"] = case([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.25], [1.0, 1.0, 3.0]], **small)
    below = np.nextafter(np.float32(2.0 ** 30), np.float32(0.0))
    cs["range_at"] = case([[0.0, 0.0, 0.0], [0.0, -2.0 ** 30, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], **small)
    cs["range_below"] = case([[0.0, 0.0, 0.0], [0.0, -below, 0.0], [below, 0.0, 0.0], [0.0, 0.0, below]], **small)
    # ---- hypothesis counts: one, and each side of the score kernel's group
    hc = planar(300)
    for h in HYPS:
        if h != N_HYP:
            cs[f"h{h}"] = case(hc, n_hyp=h)
    # ---- the threshold exactly: the sample (0,0,0), (4,0,0), (0,4,0) in some order - the seed is searched - gives |u x v| = 16 and t2q = 16 at dist
    # 0.25; a point at z = 0.25 has s*s == 16 and is an inlier, at the next float32 outward it is not
    tri = [[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]
    s_thr = seed_where(lambda s: set(sample(s, 0, 0, 4)) == {0, 1, 2})
    out = np.nextafter(np.float32(0.25), np.float32(1.0))
    cs["thr_at"] = case(tri + [[1.0, 2.0, 0.25]], dist=0.25, n_hyp=1, max_planes=1, min_inliers=3, seed=s_thr)
    cs["thr_out"] = case(tri + [[1.0, 2.0, out]], dist=0.25, n_hyp=1, max_planes=1, min_inliers=3, seed=s_thr)
    # thr_norm: the sample (0,0,0), (0,0,1), (4,-3,0) gives u x v = +-(3, 4, 0), q = 25; a point with 3 x + 4 y = 1.25 has s*s == t2q == 1.5625 and is
    # an inlier.  The point is searched so that u x v DIVIDED by its length - 0.6 and 0.8, neither exact - puts it outside
    tri2 = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [4.0, -3.0, 0.0]])
    i0, i1, i2 = sample(s_thr, 0, 0, 4)

    def normalised_leaves_out(p):
        a = tri2[i0]
        mv = np.cross(tri2[i1] - a, tri2[i2] - a)
        n = mv / np.sqrt((mv[0] * mv[0] + mv[1] * mv[1]) + mv[2] * mv[2])
        e = p - a
        t = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        return t * t > 0.25 * 0.25

    k = seed_where(lambda k_: normalised_leaves_out(np.array([k_ / 64.0, (80 - 3 * k_) / 256.0, 0.5])))
    cs["thr_norm"] = case(np.r_[tri2, [[k / 64.0, (80 - 3 * k) / 256.0, 0.5]]], dist=0.25, n_hyp=1, max_planes=1, min_inliers=3, seed=s_thr)
    # ---- score ties: an 8 x 8 lattice in one plane - every hypothesis that is not skipped scores 64; the seed is searched so that hypothesis 0 draws
    # a collinear triple (q == 0 exactly) and the first valid one wins.  Two parallel lattices of 32 points: the smaller h of the two planes' wins
    lat = np.array([[x, y, 0.0] for y in range(8) for x in range(8)], dtype=np.float64)

    def collinear(s):
        a, b, c = (lat[i] for i in sample(s, 0, 0, 64))
        return not np.cross(b - a, c - a).any()

    tie = dict(dist=0.25, n_hyp=16, max_planes=2, min_inliers=8, seed=seed_where(collinear))
    cs["coplanar"] = case(lat, **tie)
    cs["two_planes_equal"] = case(np.r_[lat[:32], lat[:32] + [0.0, 0.0, 1.0]][rng.permutation(64)], **tie)
    # ---- skipped hypotheses: nothing but duplicates, and a line - no plane; a line and one point beside it - one plane of all
    cs["all_duplicates"] = case(np.tile([[0.3, -0.2, 0.7]], (8, 1)), **tie)
    cs["on_line"] = case(np.c_[np.arange(12.0), 2.0 * np.arange(12.0), np.zeros(12)], **tie)
    cs["on_line_plus"] = case(np.r_[np.c_[np.arange(12.0), 2.0 * np.arange(12.0), np.zeros(12)], [[1.0, 0.0, 5.0]]], **tie)
    # ---- axis: a floor of 200 and a wall of 400 lattice points.  With the axis z and 10 degrees the floor wins although the wall has more points;
    # without an axis, and with cos_max_angle 0, the wall wins
    u = 1.0 / 16.0
    floor = np.array([[x * u, y * u, 0.0] for y in range(10) for x in range(20)])
    wall = np.array([[0.0 - 1.0, y * u, 1.0 + z * u] for z in range(20) for y in range(20)])
    fw = np.r_[floor, wall][rng.permutation(600)]

    def draws_from(cloud, part):
        """a seed under which one of 32 hypotheses of round 0 draws its three records from `part` (a mask), not on a line"""
        def ok(s):
            for h in range(32):
                i = sample(s, 0, h, len(cloud))
                if part[list(i)].all() and np.cross(cloud[i[1]] - cloud[i[0]], cloud[i[2]] - cloud[i[0]]).any():
                    return True
            return False
        return seed_where(ok)

    ax = dict(dist=0.03125, n_hyp=32, max_planes=1, min_inliers=50, seed=draws_from(fw, fw[:, 2] == 0.0))
    cs["floor_wall"] = case(fw, axis=(0.0, 0.0, 1.0), cos_max_angle=COS10, **ax)
    cs["floor_wall_free"] = case(fw, **ax)
    cs["floor_wall_cos0"] = case(fw, axis=(0.0, 0.0, 1.0), cos_max_angle=0.0, **ax)
    # ---- a tilted floor inside the cone (z = x / 8: 7.1 degrees) with 150 points and one outside (z = x / 4 + 3: 14.0 degrees) with 300; the axis
    # (0, 0, 2) is no unit vector: a test without aa takes the larger one
    g = np.array([[x * u, y * u] for y in range(15) for x in range(20)])
    t_in = np.c_[g[:150], g[:150, 0] / 8.0]
    t_out = np.c_[g, g[:, 0] / 4.0 + 3.0]
    tilt = np.r_[t_in, t_out][rng.permutation(450)]
    ax["seed"] = draws_from(tilt, tilt[:, 2] < 1.0)
    cs["tilt_in_out"] = case(tilt, axis=(0.0, 0.0, 2.0), cos_max_angle=COS10, **ax)
    cs["tilt_free"] = case(tilt, **ax)
    # ---- peeling: planes of 900, 500 and 200 points at z = 0, 3 and 6 and 100 scattered points between them come off in that order; round r samples
    # REMAINDER positions; max_planes cuts at 2; min_inliers 200 keeps the third plane and 201 does not
    def sheet(n, z):
        return np.c_[q12(rng.uniform(0.0, 10.0, size=(n, 2))), np.full(n, z)]

    between = np.c_[q12(rng.uniform(0.0, 10.0, size=(100, 2))), q12(np.r_[rng.uniform(0.5, 2.5, size=50), rng.uniform(3.5, 5.5, size=50)])]
    three = np.r_[sheet(900, 0.0), sheet(500, 3.0), sheet(200, 6.0), between][rng.permutation(1700)]
    pk = dict(dist=0.125, n_hyp=32)
    cs["peel"] = case(three, max_planes=4, min_inliers=200, **pk)
    cs["peel_max2"] = case(three, max_planes=2, min_inliers=200, **pk)
    cs["peel_min201"] = case(three, max_planes=4, min_inliers=201, **pk)
    cs["peel_keep_planes"] = case(three, max_planes=4, min_inliers=200, flags=KEEP_PLANES, **pk)
    # ---- m drops below 3 after a round: four points in a plane and one off it
    cs["short_after_round"] = case([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2.0, 3.0, 0.0], [0.5, 0.5, 4.0]], dist=0.25, n_hyp=16, max_planes=3, min_inliers=3)
    return cs


def load():
    """The frozen inputs of tests/golden/planecloud_cases.npz, in the table's order."""
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        ax = z[f"{n}/in/axis"]
        out[str(n)] = dict(cloud=z[f"{n}/in/cloud"], dist=float(z[f"{n}/in/dist"][0]), axis=tuple(float(v) for v in ax) if len(ax) else None,
                           cos_max_angle=float(z[f"{n}/in/cos_max_angle"][0]), **{k: int(z[f"{n}/in/{k}"][0]) for k in ("n_hyp", "max_planes", "min_inliers", "seed", "flags")})
    return out


PER_POINT = ("label", "keep")
PER_PLANE_INT = ("n_inliers", "hyp")
PER_PLANE_FLT = ("normal", "d", "centroid", "eig", "rmse")
COUNTS = ("n_on_planes", "n_rest", "n_kept", "n_planes", "status")


def golden():
    """{case: dict(label, keep per point; n_inliers, hyp, conditioned and the coefficients per plane; the counts and the status)} of the frozen file."""
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = {k: z[f"{n}/out/{k}"] for k in PER_POINT + PER_PLANE_INT + PER_PLANE_FLT + ("conditioned",)}
        g.update({k: int(z[f"{n}/out/{k}"][0]) for k in COUNTS})
        out[str(n)] = g
    return out


CASES = load() if os.path.exists(GOLDEN) else build()
NAMES = list(CASES)


def params(c):
    return tuple(c[k] for k in PARAMS)


def groups():
    """The cases that can share one call - equal parameters - as {params: [names]} in the table's order."""
    g = {}
    for n, c in CASES.items():
        g.setdefault(params(c), []).append(n)
    return g


MAIN = (DIST, N_HYP, MAX_PLANES, MIN_INLIERS, None, 0.0, SEED, 0)


def scale_of(cloud):
    v = np.abs(np.asarray(cloud, dtype=np.float64))
    return float(v.max()) if v.size else 1.0


def coefficient_errors(cloud, want, got_planes):
    """(normal, coord): the largest errors of a case's reported planes against the 50-digit values, in units of 2^-53 * scale - the normal with scale
    1 (conditioned refits only), centroid and d with the largest |coordinate|, eig and rmse^2 with its square (d on conditioned refits only)."""
    s = scale_of(cloud)
    en = ec = 0.0
    for r, p in enumerate(got_planes):
        ec = max(ec, float(np.abs(np.asarray(p["centroid"]) - want["centroid"][r]).max()) / s, float(np.abs(np.asarray(p["eig"]) - want["eig"][r]).max()) / (s * s),
                 abs(float(p["rmse"]) ** 2 - float(want["rmse"][r]) ** 2) / (s * s))
        if want["conditioned"][r]:
            en = max(en, float(np.abs(np.asarray(p["normal"]) - want["normal"][r]).max()))
            ec = max(ec, abs(float(p["d"]) - float(want["d"][r])) / s)
    return en * 2.0 ** 53, ec * 2.0 ** 53
