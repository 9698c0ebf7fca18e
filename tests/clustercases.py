"""The frozen table of clustering cases (lk_clouds_cluster_dev, lk_clouds_cluster): seeded, listed by name, small.

A case is a dict: cloud [n, 3] (float32), reach, min_pts, min_size, max_size, flags.  build() is the seeded generator; the table the tests use
(CASES) is its output as FROZEN in tests/golden/cluster_cases.npz, beside each case's expected values: n_i, kind and label per point, the size and
first core index per cluster, keep per point, the counts and the status, all from EXACT integer arithmetic on the float coordinates (a coordinate
is an integer multiple of a power of two, so every d2 is an integer).  tests/golden/make_cluster_cases.py writes the file and ASSERTS that every
decision of the table is clear:
  * membership d2 <= reach^2 by a relative 2^-40, or an exact tie (reach * reach is then exact as well);
  * the core candidate a border point joins: its d2 below the runner-up's by a relative 2^-40, or exactly equal (the smaller index is taken);
everything else is whole numbers.  So every expected value is an integer and everything is compared exactly, no case left out.
REACH_TIES names the cases in which some d2 equals reach^2 exactly, BORDER_TIES those in which a border point has two nearest core candidates at
exactly the same d2; the generator asserts that these lists are the ones it finds.  Only REACH_TIES are kept from the library yardstick of
tests/test_cluster_host.py (scikit-learn's DBSCAN and scipy's connected components take a root first): what it compares - the core set, the noise
set and the partition of the core points - does not depend on which cluster a border point joins.
"""
import os

import numpy as np

import mmecases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_cases.npz")

REACH = 0.25                    # the parameters of most cases, so that they go into one call as many clouds
MIN_PTS = 4
NO_BOUND = 0xFFFFFFFF
KEEP_LARGEST = 1
NOISE = 0xFFFFFFFF
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257]
CHAIN = 1000
DIRECTIONS = mc.DIRECTIONS
dir_name = mc.dir_name
REACH_TIES = ["chain_gap_tie"]
BORDER_TIES = ["bridge_tie", "contention"]
PARAMS = ("reach", "min_pts", "min_size", "max_size", "flags")


def case(cloud, reach=REACH, min_pts=MIN_PTS, min_size=0, max_size=NO_BOUND, flags=0):
    return dict(cloud=np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 3)), reach=float(reach), min_pts=int(min_pts), min_size=int(min_size),
                max_size=int(max_size), flags=int(flags))


def line(xs, y=0.0, z=0.0):
    xs = np.asarray(xs, dtype=np.float64)
    return np.c_[xs, np.full(len(xs), y), np.full(len(xs), z)]


def blob(rng, n, at):
    """n points within 0.03 of `at`: all within reach of each other"""
    return np.asarray(at) + rng.uniform(-0.015, 0.015, size=(n, 3))


def build():
    rng = np.random.default_rng(20261022)
    cs = {}
    box = lambda n, side: rng.uniform(-side / 2, side / 2, size=(n, 3))   # noqa: E731
    dense = lambda n: box(n, 0.22 * max(n, 1) ** (1.0 / 3.0))              # noqa: E731  about 6 neighbours within 0.25 m: core, border and noise points
    # ---- sizes: nothing, a point, a pair, a wave, a block and their neighbours.  The invalid clouds and the empty one stand in the middle of the call
    for n in SIZES[:5]:
        cs[f"s{n}"] = case(dense(n))
    good = box(60, 0.6)
    for name, value in (("nan_cloud", np.nan), ("inf_cloud", -np.inf)):
        c = good.copy()
        c[11, 1] = value
        cs[name] = case(c)
    cs["empty_mid"] = case(np.zeros((0, 3)))
    for n in SIZES[5:]:
        cs[f"s{n}"] = case(dense(n))
    # ---- chain: 1 000 points in a line spaced just under the reach (1023 / 1024 of it: every coordinate exact) - one cluster, deep parent paths - in
    # ascending, descending and shuffled index order; with one gap at d2 == reach^2 exactly (one cluster) and at the next float outward (two)
    s = REACH * (1.0 - 2.0 ** -10)
    xs = np.arange(CHAIN) * s
    cs["chain_asc"] = case(line(xs), min_pts=2)
    cs["chain_desc"] = case(line(xs[::-1]), min_pts=2)
    cs["chain_shuffled"] = case(line(rng.permutation(xs)), min_pts=2)
    half = CHAIN // 2
    tie = xs.copy()
    tie[half:] += REACH - s
    assert np.array_equal(tie.astype(np.float32).astype(np.float64), tie) and tie[half] - tie[half - 1] == REACH
    cs["chain_gap_tie"] = case(line(tie), min_pts=2)
    start = np.nextafter(np.float32(xs[half - 1] + REACH), np.float32(np.inf)).astype(np.float64)
    cs["chain_gap_out"] = case(line(np.r_[xs[:half], start + np.arange(CHAIN - half) * s]), min_pts=2)
    cs["many"] = case(np.array([[x, y, 0.0] for y in range(64) for x in range(64) for _ in (0, 1)], dtype=np.float64)
                      + np.tile([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0]], (4096, 1)), min_pts=2)    # 4 096 two-point clusters
    cs["mp2"] = case(dense(40), min_pts=2)
    # ---- bridge: two core groups (four points 3/64 apart each) joined only through one point that sees one core point of each - 15/64 from A's last,
    # 14/64 from B's first - and so has n = 3 < min_pts: two clusters, and the point joins B, the nearer, although A's index is the smaller.
    # bridge_tie: 15/64 from both, B listed first: it joins the smaller core index.  numbering: the point listed first - cluster 1's border
    u = 1.0 / 64.0
    A = line(np.array([-9, -6, -3, 0]) * u)
    cs["bridge"] = case(np.r_[A, line(np.array([29, 32, 35, 38]) * u), line([15 * u])])
    cs["bridge_tie"] = case(np.r_[line(np.array([30, 33, 36, 39]) * u), A, line([15 * u])])
    cs["numbering"] = case(np.r_[line([15 * u]), A, line(np.array([29, 32, 35, 38]) * u)])
    # ---- min_pts: 1 (no noise, no border: the connected components), the cloud's size (12 points within reach of each other: all core), one above
    # it (all noise)
    cs["mp1"] = case(dense(40), min_pts=1)
    tight = box(12, 0.1)
    cs["mp_n"] = case(tight, min_pts=12)
    cs["mp_n1"] = case(tight, min_pts=13)
    # ---- duplicates: a point copied three times is core by its copies alone, a single one far away is noise; a cloud of nothing but duplicates
    cs["duplicates"] = case(np.r_[np.tile([[0.3, -0.2, 0.7]], (4, 1)), [[3.0, 3.0, 3.0]], [[0.3, -0.2, 0.7 + 0.2]]])
    cs["all_duplicates"] = case(np.tile([[0.3, -0.2, 0.7]], (8, 1)))
    # ---- cell geometry, at min_pts 1: the query and one point in each of the 26 cells around its own in turn, linked through that cell alone; two
    # cells away no link; c2ccases.py's row-wrap trap (A's x range stops at the grid's edge: B, first cell of the next row, is not looked at)
    q0 = np.array([0.125, 0.125, 0.125])
    anchors = [[-0.65, -0.65, -0.65], [0.65, 0.65, 0.65]]
    for d in DIRECTIONS:
        cs[dir_name(d)] = case(np.r_[[q0], anchors, [q0 + 0.135 * np.array(d)]], min_pts=1)
    cs["two_cells_away"] = case(np.r_[[[0.245, 0.125, 0.125]], anchors, [[0.505, 0.125, 0.125]]], min_pts=1)
    cs["wrap_trap"] = case([[1.45, 0.125, 0.125], [0.05, 0.375, 0.125], [1.40, 0.13, 0.12]], min_pts=1)
    # ---- size filter, at min_pts 1: clusters of 3, 5, 8, 8 and 9 points.  Bounds 5 .. 8: a size at min_size, two at max_size, one outside each;
    # KEEP_LARGEST there: two of equal size, the smaller id; KEEP_LARGEST with bounds nobody meets; KEEP_LARGEST without bounds
    blobs = np.concatenate([blob(rng, n, [float(k), 0.0, 0.0]) for k, n in enumerate((3, 8, 5, 9, 8))])
    cs["sf_bounds"] = case(blobs, min_pts=1, min_size=5, max_size=8)
    cs["sf_largest_tie"] = case(blobs, min_pts=1, min_size=5, max_size=8, flags=KEEP_LARGEST)
    cs["sf_largest_none"] = case(blobs, min_pts=1, min_size=10, max_size=20, flags=KEEP_LARGEST)
    cs["sf_largest"] = case(blobs, min_pts=1, flags=KEEP_LARGEST)
    # ---- shared cells: two combs, backbones 2 m apart, teeth 0.5 m apart reaching for the other's backbone; a tooth of one and a tooth of the other
    # lie in the same cells (x 0.02 / 0.23, z 0.01 / 0.24) and 0.31 m apart
    ticks = np.arange(0.0, 2.05, 0.1)
    comb_a = [line(ticks, 0.0, 0.01)] + [np.c_[np.full(17, 0.02 + 0.5 * k), 0.1 + 0.1 * np.arange(17), np.full(17, 0.01)] for k in range(4)]
    comb_b = [line(ticks, 2.0, 0.24)] + [np.c_[np.full(17, 0.23 + 0.5 * k), 1.9 - 0.1 * np.arange(17), np.full(17, 0.24)] for k in range(4)]
    cs["combs"] = case(np.concatenate(comb_a + comb_b)[rng.permutation(2 * (21 + 4 * 17))])
    # ---- cloud boundaries: two clouds of one call with identical coordinates
    twin = dense(65)
    cs["boundary_a"] = case(twin)
    cs["boundary_b"] = case(twin)
    # ---- range: clusters 3 km apart under reach 0.05 (the edge has to double); |p / reach| at 2^30 and one float below
    far = np.array([1800.0, 1800.0, 1600.0])
    cs["far_clusters"] = case(np.r_[rng.uniform(0.0, 0.15, size=(64, 3)), far + rng.uniform(0.0, 0.15, size=(64, 3))], reach=0.05)
    rr = 2.0 ** -10
    cs["range_at"] = case([[0.0, 0.0, 0.0], [0.0, -2.0 ** 20, 0.0], [0.0, 0.0, 0.0005]], reach=rr, min_pts=1)
    inside = np.nextafter(np.float32(2.0 ** 20), np.float32(0.0))
    cs["range_below"] = case([[0.0, 0.0, 0.0], [inside, 0.0, 0.0005], [0.0, 0.0, 0.0005], [inside, 0.0, 0.0]], reach=rr, min_pts=1)
    # ---- contention: a 200 x 100 plane lattice at 0.8 reach (0.25 under reach 0.3125: every coordinate exact) - every union meets one root.  The
    # four corners have three neighbours: border points, each with two core candidates at the same distance
    cs["contention"] = case(np.array([[0.25 * x, 0.25 * y, 0.0] for y in range(100) for x in range(200)]), reach=0.3125)
    return cs


def load():
    """The frozen inputs of tests/golden/cluster_cases.npz, in the table's order."""
    z = np.load(GOLDEN)
    return {str(n): dict(cloud=z[f"{n}/in/cloud"], reach=float(z[f"{n}/in/reach"][0]), **{k: int(z[f"{n}/in/{k}"][0]) for k in PARAMS[1:]}) for n in z["names"]}


PER_POINT = ("n", "kind", "label", "keep")
PER_CLUSTER = ("cl_size", "cl_first")
COUNTS = ("n_core", "n_border", "n_noise", "n_kept", "n_clusters", "n_kept_clusters", "largest", "largest_size", "status")


def golden():
    """{case: dict(n, kind, label, keep per point; cl_size, cl_first per cluster; the counts and the status)} of the frozen file."""
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = {k: z[f"{n}/out/{k}"] for k in PER_POINT + PER_CLUSTER}
        g.update({k: int(z[f"{n}/out/{k}"][0]) for k in COUNTS})
        out[str(n)] = g
    return out


CASES = load() if os.path.exists(GOLDEN) else build()
NAMES = list(CASES)


def params(c):
    return tuple(c[k] for k in PARAMS)


def groups():
    """The cases that can share one call - equal parameters - as {(reach, min_pts, min_size, max_size, flags): [names]} in the table's order."""
    g = {}
    for n, c in CASES.items():
        g.setdefault(params(c), []).append(n)
    return g


MAIN = (REACH, MIN_PTS, 0, NO_BOUND, 0)
