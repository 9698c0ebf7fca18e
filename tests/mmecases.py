"""The frozen table of map-entropy cases (lk_clouds_mme_dev, lk_clouds_mme): seeded, listed by name, small.

A case is a dict: cloud [n, 3] (float32), radius, min_pts.  build() is the seeded generator; the table the tests use (CASES) is its output as FROZEN
in tests/golden/mme_cases.npz, beside each case's expected values: n_i, the class of every point, n_pairs, worst and the status from EXACT integer
arithmetic on the float coordinates (a coordinate is an integer multiple of a power of two, so the offsets about a point, their products, the sums
s and M and n M - s s^T are integers), and h_i, lmin_i, kappa_i = (tr / 3)^3 / det, mme, mpv, h_max evaluated from those integers with mpmath at 50
digits and rounded to float64.  tests/golden/make_mme_cases.py writes the file and ASSERTS that every decision of the table is clear:
  * membership d2 <= r^2 by a relative 2^-40, or an exact tie (r * r is then exact as well);
  * n_i against min_pts: integers;
  * flatness: det / (tr / 3)^3 at most a quarter of the floor 2^-30 or at least four times it;
  * worst: the largest h leads the runner-up by four times its tolerance, or the two are duplicates of one point (equal bits by construction);
so counts, classes and worst are compared exactly, no case left out.  tests/test_mme_host.py checks that the values regenerate to the bit from the
frozen inputs and that build() still gives those inputs.

TOLERANCE, per point:  |lmin_dev - lmin_50| <= C_L * 2^-53 * r^2;  |h_dev - h_50| <= C_H * 2^-53 * (kappa_i + |h_i|).
The offsets are bounded by r, so C carries rounding of order 2^-53 r^2, and the eigenvalue routine a few ulp of the largest eigenvalue (< r^2).
h = const + ln(det) / 2: the relative rounding of det is that of C over its smallest eigenvalue, which kappa_i bounds up to a small factor; |h_i|
stands for the rounding of the logarithm and the final sum.  Per cloud: mpv as a point's lmin, mme the mean of its scored points' bounds, h_max the
bound of the worst point.
C = 16 * max(1, worst ratio error / (bound at C = 1) that legkilo_amd.cloudmetrics.mme reaches over this table): the factor 16 covers another
summation order and another eigenvalue routine (tests/c2ccases.py reasons the same way).  Measured on this table by make_mme_cases.py:
    NUMPY_RATIO_H = 35.64   ("heavy_cell", h of point 742: 700 terms per sum, added one after the other as the device adds them - the bound has
                             no term for the length of a sum, so the crowded cell sets the ratio)
    NUMPY_RATIO_L = 14.19   ("heavy_cell", lmin of point 604, for the same reason)
so C_H = 570.2, C_L = 227.0.  tests/test_mme_host.py re-measures both and fails if one exceeds twice its recorded value.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mme_cases.npz")
NUMPY_RATIO_H = 35.64
NUMPY_RATIO_L = 14.19
C_H = 16.0 * max(1.0, NUMPY_RATIO_H)
C_L = 16.0 * max(1.0, NUMPY_RATIO_L)
ULP = 2.0 ** -53
FLOOR = 2.0 ** -30
SPARSE, FLAT, SCORED = 0, 1, 2

R = 0.25                        # radius of most cases, so that they go into one call as many clouds
MIN_PTS = 5
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 257]
DIRECTIONS = [(a, b, c) for c in (-1, 0, 1) for b in (-1, 0, 1) for a in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
TETRA = 0.003 * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])


def case(cloud, radius=R, min_pts=MIN_PTS):
    return dict(cloud=np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 3)), radius=float(radius), min_pts=int(min_pts))


def dir_name(d):
    return "dir_" + "".join("m0p"[v + 1] for v in d)


def build():
    rng = np.random.default_rng(20261022)
    cs = {}
    box = lambda n, lo=-0.6, hi=0.6: rng.uniform(lo, hi, size=(n, 3))   # noqa: E731
    # ---- sizes: uniform points in a 1.2 m box (125 cells of 0.25 m): below, at and above min_pts, a wave, a block and their neighbours
    for n in SIZES:
        cs[f"s{n}"] = case(box(n))
    # ---- density: a centre with min_pts - 2 satellites (n = 4: sparse) beside one with min_pts - 1 (n = 5: dense), 2 m apart; the satellites lie
    # 0.2 m out in tetrahedral directions, 0.327 m from each other, so each of them sees the centre alone
    sat = 0.2 / np.sqrt(3.0) * (TETRA / 0.003)
    cs["density_edge"] = case(np.r_[[[0.0, 0.0, 0.0]], sat[:3] * [1.0, 0.9, 1.1], [[2.0, 2.0, 2.0]], 2.0 + sat * [1.0, 0.9, 1.1]])
    # ---- reach: d2 == r^2 exactly is a member (3-4-5 at 5 * 2^-4), the next float outward is not; three points near the origin make it dense
    e = 2.0 ** -4
    out4 = np.nextafter(np.float32(4 * e), np.float32(np.inf))
    cs["reach_exact"] = case([[0.0, 0.0, 0.0], [3 * e, 4 * e, 0.0], [-3 * e, -out4, 0.0], [0.0, 0.0, 5 * e], [0.01, 0.02, 0.03], [-0.02, 0.01, 0.015],
                              [0.015, -0.01, -0.02]], radius=5 * e)
    # ---- neighbour direction: a four-point cluster within reach in each of the 26 cells around the query's; two anchors span a 6-cell grid.  The
    # query has n = 6 = min_pts of these cases - the cluster, itself and a point of its own cell on the far side, which the cluster does not reach -
    # so a cell left out shows in n and in the class, and the query is the only dense point (five points that all see each other would tie in h)
    q0 = np.array([0.125, 0.125, 0.125])
    anchors = [[-0.65, -0.65, -0.65], [0.65, 0.65, 0.65]]
    for d in DIRECTIONS:
        cs[dir_name(d)] = case(np.r_[[q0], anchors, q0 + 0.135 * np.array(d) + TETRA, [q0 - 0.12 * np.array(d)]], min_pts=6)
    cs["two_cells_away"] = case(np.r_[[[0.245, 0.125, 0.125]], anchors, [0.505, 0.125, 0.125] + TETRA])   # cell 2 against cell 0, d > 0.257
    # the wrap trap of c2ccases.py: A at the x-max end of a row, B at the x-min end of the next row - A's x range must stop at the grid's edge
    cs["wrap_trap"] = case([[1.45, 0.125, 0.125], [0.05, 0.375, 0.125], [1.40, 0.13, 0.12]])
    # ---- one crowded cell: 600 points inside a single cell, two anchors, and 150 points over the 27 cells around it: without those the points in
    # the cell's middle would all see the same 600 records and tie in h
    cs["heavy_cell"] = case(np.r_[anchors, rng.uniform(0.02, 0.23, size=(600, 3)), rng.uniform(-0.25, 0.5, size=(150, 3))])
    # ---- coordinates within 1e-6 of 0 on both sides (floor, not truncation), duplicates, nothing but duplicates
    tiny = np.array([[sx * 1e-7, sy * 3e-7, sz * 5e-7] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    cs["around_zero"] = case(np.r_[tiny, box(100, -0.3, 0.3), tiny * 1.5])
    base = box(40, -0.25, 0.25)
    cs["duplicates"] = case(np.r_[base, base[[3, 3, 17, 5]], base[:2]])
    cs["all_duplicates"] = case(np.tile([[0.3, -0.2, 0.7]], (8, 1)))
    # ---- far-apart clusters: 3 km apart under r = 0.05 - 36 000 x 36 000 x 32 000 cells of 0.05 m, so the edge has to double
    far = np.array([1800.0, 1800.0, 1600.0])
    cs["far_clusters"] = case(np.r_[rng.uniform(0.0, 0.15, size=(64, 3)), far + rng.uniform(0.0, 0.15, size=(64, 3))], radius=0.05)
    # (towards the corners of a 9.8 m cube: points that all see each other, or a middle that sees everything, would tie in h)
    cs["one_cell"] = case(np.where(rng.uniform(size=(50, 3)) < 0.5, rng.uniform(0.1, 2.0, size=(50, 3)), rng.uniform(8.0, 9.9, size=(50, 3))), radius=10.0)
    # ---- planes, a line, flatness
    xy = lambda n: rng.uniform(0.0, 1.0, size=(n, 2))   # noqa: E731
    p = xy(150)
    cs["plane_noise_1cm"] = case(np.c_[p, 0.3 + rng.normal(0.0, 0.01, size=150)])
    p = xy(150)
    cs["tilted_plane_1mm"] = case(np.c_[p, 0.2 * p[:, 0] + 0.3 * p[:, 1] + rng.normal(0.0, 0.001, size=150)])   # det / (tr/3)^3 about 1e-4
    cs["plane_exact"] = case(np.c_[xy(150), np.full(150, 0.25)])                                                 # det == 0.0 to the bit: flat
    p = xy(150)
    cs["plane_f32_at_50m"] = case(np.c_[50.0 + p[:, 0], 60.0 + p[:, 1], 2.0 + 0.2 * p[:, 0] + 0.3 * p[:, 1]], radius=0.3)   # flat by storage rounding
    t = rng.uniform(0.0, 1.0, size=(40, 1))
    cs["line"] = case(np.array([0.1, 0.2, 0.3]) + t * np.array([0.8, 0.4, 0.2]))
    # ---- far from the origin
    cs["box_far"] = case(np.array([3000.0, 2000.0, 100.0]) + box(200))
    # ---- status: NaN, inf, a coordinate at |p / r| = 2^30 exactly, and the largest one that is still in range
    good = box(60, -0.3, 0.3)
    for name, value in (("nan_cloud", np.nan), ("inf_cloud", -np.inf)):
        c = good.copy()
        c[11, 1] = value
        cs[name] = case(c)
    rr = 2.0 ** -10
    cs["range_at"] = case([[0.0, 0.0, 0.0], [0.0, -2.0 ** 20, 0.0], [0.0, 0.0, 0.0005]], radius=rr)
    inside = np.nextafter(np.float32(2.0 ** 20), np.float32(0.0))
    cs["range_below"] = case([[0.0, 0.0, 0.0], [inside, 0.0, 0.0005], [0.0, 0.0, 0.0005], [inside, 0.0, 0.0]], radius=rr)
    return cs


def load():
    """The frozen inputs of tests/golden/mme_cases.npz, in the table's order."""
    z = np.load(GOLDEN)
    return {str(n): dict(cloud=z[f"{n}/in/cloud"], radius=float(z[f"{n}/in/radius"][0]), min_pts=int(z[f"{n}/in/min_pts"][0])) for n in z["names"]}


PER_POINT = ("n", "cls", "h", "lmin", "kappa")
FIGURES = ("mme", "mpv", "h_max")
COUNTS = ("n_dense", "n_scored", "n_pairs", "worst", "status")


def golden():
    """{case: dict(n, cls, h, lmin, kappa per point; mme, mpv, h_max; n_dense, n_scored, n_pairs, worst, status)} of the frozen file."""
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = {k: z[f"{n}/out/{k}"] for k in PER_POINT}
        g.update({k: float(z[f"{n}/out/{k}"][0]) for k in FIGURES})
        g.update({k: int(z[f"{n}/out/{k}"][0]) for k in COUNTS})
        out[str(n)] = g
    return out


CASES = load() if os.path.exists(GOLDEN) else build()
NAMES = list(CASES)


def tol_lmin(c, ratio=None):
    return (C_L if ratio is None else ratio) * ULP * c["radius"] * c["radius"]


def tol_h(g, ratio=None):
    """Per point, NaN where the point is not scored."""
    return (C_H if ratio is None else ratio) * ULP * (g["kappa"] + np.abs(g["h"]))


def tol_record(c, g, ratio_h=None, ratio_l=None):
    """(mme, mpv, h_max) bounds of a case's record."""
    th = tol_h(g, ratio_h)
    sc = g["cls"] == SCORED
    return (float(th[sc].mean()) if sc.any() else 0.0, tol_lmin(c, ratio_l), float(th[g["worst"]]) if sc.any() else 0.0)


def groups():
    """The cases that can share one call - equal radius and min_pts - as {(radius, min_pts): [names]} in the table's order."""
    g = {}
    for n, c in CASES.items():
        g.setdefault((c["radius"], c["min_pts"]), []).append(n)
    return g
