"""The frozen table of outlier-filter cases (lk_clouds_sor_dev, lk_clouds_sor): seeded, listed by name, small.

A case is a dict: cloud [n, 3] (float32), k, reach, n_sigma.  build() is the seeded generator; the table the tests use (CASES) is its output as FROZEN
in tests/golden/sor_cases.npz, beside each case's expected values: cnt_i, keep_i, the counts, worst and the status from EXACT integer arithmetic on
the float coordinates (a coordinate is an integer multiple of a power of two, so every d2 is an integer, and the k smallest of them are found without
rounding), and dbar_i, mu, sigma, thr evaluated from those integers with mpmath at 50 digits and rounded to float64.
tests/golden/make_sor_cases.py writes the file and ASSERTS that every decision of the table is clear:
  * membership d2 <= reach^2 by a relative 2^-40, or an exact tie (reach * reach is then exact as well);
  * cnt_i against k: integers;
  * every non-isolated dbar_i at least 2^10 tolerances (of dbar plus of thr) away from thr, or equal to it as a rational number (duplicates);
  * worst: the largest dbar leads the runner-up by four times its tolerance, or the two are equal as exact numbers and the first index is taken;
so keep, cnt, the counts, worst, status, the output offsets, the output records and src_idx are compared exactly, no case left out.

TOLERANCE.  |dbar_dev - dbar_50| and |mu_dev - mu_50| <= C_D * 2^-53 * reach;  |sigma_dev - sigma_50| and |thr_dev - thr_50| <= C_S * 2^-53 *
(reach + reach^2 / sigma_50), and exactly equal where sigma_50 == 0 or thr is +inf.
Every d2 is bounded by reach^2 and carries three roundings, its root one more, the k-term sum k - 1 and the division one: dbar is a few 2^-53 reach
off.  mu adds the length of its lane's sum.  sigma is the root of a sum of squares of differences from mu: an error e in mu or dbar moves sum (d - mu)^2
by at most 2 e sum |d - mu|, which against sigma is of order e * reach / sigma - the second term of the unit.
C = 16 * max(1, worst ratio error / (bound at C = 1) that legkilo_amd.cloudmetrics.sor reaches over this table), the project's rule (tests/mmecases.py).
Measured on this table by make_sor_cases.py:
    NUMPY_RATIO_D = 3.00   ("k32", dbar of point 66: 32 roots added one after the other - the unit has no term for the length of the sum)
    NUMPY_RATIO_S = 0.151  ("duplicates", thr)
so C_D = 48, C_S = 16.  tests/test_sor_host.py re-measures both and fails if one exceeds twice its recorded value.
"""
import os

import numpy as np

import mmecases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sor_cases.npz")
NUMPY_RATIO_D = 3.00
NUMPY_RATIO_S = 0.151
C_D = 16.0 * max(1.0, NUMPY_RATIO_D)
C_S = 16.0 * max(1.0, NUMPY_RATIO_S)
ULP = 2.0 ** -53

K = 4                           # k, reach and n_sigma of most cases, so that they go into one call as many clouds
REACH = 0.25
N_SIGMA = 2.0
SIZES = [0, 1, K, K + 1, K + 2, 63, 64, 65, 255, 257]
CAPS = (8, 16, 32)              # the list capacities of lk_sor.h
DIRECTIONS = mc.DIRECTIONS
dir_name = mc.dir_name
TETRA = mc.TETRA


def case(cloud, k=K, reach=REACH, n_sigma=N_SIGMA):
    return dict(cloud=np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 3)), k=int(k), reach=float(reach), n_sigma=float(n_sigma))


def build():
    rng = np.random.default_rng(20261021)
    cs = {}
    box = lambda n, side: rng.uniform(-side / 2, side / 2, size=(n, 3))   # noqa: E731
    dense = lambda n: box(n, 0.18 * max(n, 1) ** (1.0 / 3.0))              # noqa: E731  about 11 neighbours within 0.25 m
    # ---- sizes: below, at and above k + 1 (the smallest cloud with a point that is not isolated), a wave, a block and their neighbours
    for n in SIZES:
        cs[f"s{n}"] = case(dense(n))
    # ---- k: the smallest, the largest, and one above each list capacity (the next instantiation takes over)
    cs["k1"] = case(dense(65), k=1)
    cs["k9"] = case(dense(255), k=CAPS[0] + 1)
    cs["k17"] = case(box(257, 0.9), k=CAPS[1] + 1)
    cs["k32"] = case(box(257, 0.75), k=CAPS[2])
    # ---- reach: d2 == reach^2 exactly is a candidate (3-4-5 at 5 * 2^-4), the next float outward is not.  The origin has k = 3 candidates with
    # the tie and two without
    e = 2.0 ** -4
    out4 = np.nextafter(np.float32(4 * e), np.float32(np.inf))
    cs["reach_exact"] = case([[0.0, 0.0, 0.0], [3 * e, 4 * e, 0.0], [-3 * e, -out4, 0.0], [0.01, 0.02, 0.03], [-0.02, 0.01, 0.015]], k=3, reach=5 * e)
    # ---- neighbour direction (mmecases.py's): a four-point cluster within reach in each of the 26 cells around the query's and one point of the
    # query's own cell; the query has k = 5 candidates - a cell left out shows in cnt and flips it from kept to isolated - and is the only point
    # that is not isolated: n_s == 1, sigma == 0
    q0 = np.array([0.125, 0.125, 0.125])
    anchors = [[-0.65, -0.65, -0.65], [0.65, 0.65, 0.65]]
    for d in DIRECTIONS:
        cs[dir_name(d)] = case(np.r_[[q0], anchors, q0 + 0.135 * np.array(d) + TETRA, [q0 - 0.12 * np.array(d)]], k=5)
    cs["two_cells_away"] = case(np.r_[[[0.245, 0.125, 0.125]], anchors, [0.505, 0.125, 0.125] + TETRA], k=3)   # cell 2 against cell 0, d > 0.257
    cs["wrap_trap"] = case([[1.45, 0.125, 0.125], [0.05, 0.375, 0.125], [1.40, 0.13, 0.12]], k=1)              # A's x range stops at the grid's edge
    # ---- one crowded cell at k = 32: 600 points inside a single cell, two anchors, 150 points over the 27 cells around it - the list churns
    cs["heavy_cell"] = case(np.r_[anchors, rng.uniform(0.02, 0.23, size=(600, 3)), rng.uniform(-0.25, 0.5, size=(150, 3))], k=32)
    # ---- coordinates within 1e-6 of 0 on both sides (floor, not truncation), duplicates, nothing but duplicates
    tiny = np.array([[sx * 1e-7, sy * 3e-7, sz * 5e-7] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    cs["around_zero"] = case(np.r_[tiny, box(100, 0.6), tiny * 1.5])
    base = box(40, 0.5)
    cs["duplicates"] = case(np.r_[base, base[[3, 3, 17, 5]], base[:2]], k=1)   # a copy is a candidate at distance 0; the point itself is none
    cs["all_duplicates"] = case(np.tile([[0.3, -0.2, 0.7]], (8, 1)))
    # ---- far-apart clusters: 3 km apart under reach = 0.05, so the edge has to double
    far = np.array([1800.0, 1800.0, 1600.0])
    cs["far_clusters"] = case(np.r_[rng.uniform(0.0, 0.15, size=(64, 3)), far + rng.uniform(0.0, 0.15, size=(64, 3))], reach=0.05)
    # ---- statistics: one point in them; n_sigma = 0 and +inf on one cloud
    cs["one_in_stats"] = case([[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [-0.2, 0.0, 0.0]], k=2)
    cloud = dense(65)
    cs["nsigma_zero"] = case(cloud, n_sigma=0.0)
    cs["nsigma_inf"] = case(cloud, n_sigma=np.inf)
    # ---- strays: a jittered lattice patch of 257 points (0.1 m), four points farther than reach from everything (isolated), and a loose clump - a
    # tetrahedron of edge 0.24 m and its centre - whose points see each other (not isolated) at twice the patch's spacing (statistical outliers)
    grid = np.array([[x, y, z] for z in range(6) for y in range(7) for x in range(7)], dtype=np.float64)[:257] * 0.1
    patch = grid + rng.uniform(-0.02, 0.02, size=grid.shape)
    lone = np.array([[1.5, 0.3, 0.2], [-0.6, 0.2, 0.3], [0.3, 1.4, 0.1], [0.3, 0.3, 1.3]])
    clump = np.array([2.0, 2.0, 2.0]) + np.r_[TETRA / 0.003 * (0.24 / np.sqrt(8.0)), [[0.0, 0.0, 0.0]]]
    cs["strays"] = case(np.r_[patch, lone, clump])
    # ---- sigma_edge: k = 1, three pairs 0.1 m apart and a seventh point 0.3 m from a pair.  Its dbar - mu is 6 x / 7 (x = 0.2), sigma is x / sqrt 7
    # under the divisor n_s - 1 and x sqrt 6 / 7 under n_s: kept for n_sigma >= 2.268 and >= 2.449.  2.35 lies between
    cs["sigma_edge"] = case([[0.0, 0, 0], [0.1, 0, 0], [5.0, 0, 0], [5.1, 0, 0], [10.0, 0, 0], [10.1, 0, 0], [10.4, 0, 0]], k=1, reach=1.0, n_sigma=2.35)
    # ---- status: NaN, inf, a coordinate at |p / reach| = 2^30 exactly, and the largest one that is still in range
    good = box(60, 0.6)
    for name, value in (("nan_cloud", np.nan), ("inf_cloud", -np.inf)):
        c = good.copy()
        c[11, 1] = value
        cs[name] = case(c)
    rr = 2.0 ** -10
    cs["range_at"] = case([[0.0, 0.0, 0.0], [0.0, -2.0 ** 20, 0.0], [0.0, 0.0, 0.0005]], k=1, reach=rr)
    inside = np.nextafter(np.float32(2.0 ** 20), np.float32(0.0))
    cs["range_below"] = case([[0.0, 0.0, 0.0], [inside, 0.0, 0.0005], [0.0, 0.0, 0.0005], [inside, 0.0, 0.0]], k=1, reach=rr)
    return cs


def load():
    """The frozen inputs of tests/golden/sor_cases.npz, in the table's order."""
    z = np.load(GOLDEN)
    return {str(n): dict(cloud=z[f"{n}/in/cloud"], k=int(z[f"{n}/in/k"][0]), reach=float(z[f"{n}/in/reach"][0]), n_sigma=float(z[f"{n}/in/n_sigma"][0]))
            for n in z["names"]}


PER_POINT = ("cnt", "keep", "dbar")
FIGURES = ("mu", "sigma", "thr")
COUNTS = ("n_isolated", "n_outliers", "n_kept", "worst", "status")


def golden():
    """{case: dict(cnt, keep, dbar per point; mu, sigma, thr; n_isolated, n_outliers, n_kept, worst, status)} of the frozen file."""
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


def tol_d(c, ratio=None):
    """dbar and mu"""
    return (C_D if ratio is None else ratio) * ULP * c["reach"]


def tol_s(c, g, ratio=None):
    """sigma and thr; 0 where sigma_50 is 0 or NaN (compared exactly)"""
    s = g["sigma"]
    return (C_S if ratio is None else ratio) * ULP * (c["reach"] + c["reach"] * c["reach"] / s) if s > 0.0 else 0.0


def groups():
    """The cases that can share one call - equal k, reach and n_sigma - as {(k, reach, n_sigma): [names]} in the table's order."""
    g = {}
    for n, c in CASES.items():
        g.setdefault((c["k"], c["reach"], c["n_sigma"]), []).append(n)
    return g
