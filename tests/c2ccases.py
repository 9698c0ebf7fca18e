"""The frozen table of cloud-to-cloud cases (lk_clouds_c2c_dev, lk_clouds_c2c): seeded, listed by name, small.

A case is a dict: query [n, 3], ref [m, 3] (float32), max_dist, thr (float64, up to four).  build() is the seeded generator; the table the tests use
(CASES) is its output as FROZEN in tests/golden/c2c_cases.npz, beside each case's expected values: j(i), the matched flags, n_within, worst and the
status from exact comparisons at 50 digits, rmse / mean / max evaluated at 50 digits from the float coordinates and rounded to float64.
tests/golden/make_c2c_cases.py writes the file and ASSERTS, at 50 digits, that every decision of the table is either clear by a relative 2^-40 or an
exact tie whose rounded float64 values are equal as well - so indices, flags and counts are compared exactly, no case left out.
tests/test_c2c_host.py checks that the values regenerate to the bit from the frozen inputs and that build() still gives those inputs.

TOLERANCE.  |x_dev - x_50| <= C * 2^-53 * max_dist for rmse, mean and max (every d_i is at most max_dist).
C = 16 * max(1, worst ratio |x_numpy - x_50| / (2^-53 * max_dist) that legkilo_amd.cloudmetrics.c2c reaches over this table): the factor 16 covers
another summation order (tests/atecases.py reasons the same way).  Measured on this table, all three figures:
    NUMPY_RATIO = 1.0   (1.000 on "s63_64" and "s65_63", rmse: one ulp of a figure in [0.125, 0.25), the final sqrt and division; numpy's pairwise sums add
                         nothing visible; the device reaches 2.0)
so C = 16.  tests/test_c2c_host.py re-measures the ratio and fails if it exceeds twice NUMPY_RATIO.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2c_cases.npz")
NUMPY_RATIO = 1.0
C = 16.0 * max(1.0, NUMPY_RATIO)
ULP = 2.0 ** -53
NO_MATCH = 0xFFFFFFFF

M = 0.25                        # max_dist of most cases, so that they go into one call as many pairs
THR = (0.05, 0.125, 0.25)
SIZES = [(0, 0), (0, 65), (65, 0), (1, 1), (2, 2), (63, 64), (64, 65), (65, 63), (257, 257), (1, 257), (257, 1)]   # (query, reference)
DIRECTIONS = [(a, b, c) for c in (-1, 0, 1) for b in (-1, 0, 1) for a in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
FACES = {"xp": (0, 1), "xm": (0, -1), "yp": (1, 1), "ym": (1, -1), "zp": (2, 1), "zm": (2, -1)}


def case(query, ref, max_dist=M, thr=THR):
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))   # noqa: E731
    return dict(query=f(query), ref=f(ref), max_dist=float(max_dist), thr=np.asarray(thr, dtype=np.float64).reshape(-1))


def dir_name(d):
    return "dir_" + "".join("m0p"[v + 1] for v in d)


def build():
    rng = np.random.default_rng(20261021)
    cs = {}
    box = lambda n, lo=-0.6, hi=0.6: rng.uniform(lo, hi, size=(n, 3))   # noqa: E731
    # ---- sizes: uniform points in a 1.2 m box (125 cells of 0.25 m and their neighbours): some matched, some not
    for nq, nr in SIZES:
        cs[f"s{nq}_{nr}"] = case(box(nq), box(nr))
    # ---- neighbour direction: the only reference point in reach lies in each of the 26 cells around the query's; two anchors span a 6-cell grid
    q0 = np.array([0.125, 0.125, 0.125])
    anchors = [[-0.65, -0.65, -0.65], [0.65, 0.65, 0.65]]
    for d in DIRECTIONS:
        cs[dir_name(d)] = case([q0], anchors + [q0 + 0.135 * np.array(d)])
    cs["in_block_out_of_reach"] = case([q0], anchors + [q0 + [0.225, 0.225, 0.0]])     # cell (1, 1, 0) of the block, d = 0.318
    cs["two_cells_away"] = case([[0.245, 0.125, 0.125]], anchors + [[0.505, 0.125, 0.125]])   # cell 2 against cell 0, d = 0.26
    # ---- a query outside the reference's bounding box, beyond each face: 0.1 m out (in reach of the face's points), 0.3 m and 10 m out (not)
    lattice = np.stack(np.meshgrid(*[np.linspace(0.0, 1.0, 5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.01, 0.01, size=(125, 3))
    for name, (axis, sign) in FACES.items():
        q = np.tile([0.52, 0.47, 0.55], (3, 1))
        q[:, axis] = [1.11, 1.31, 11.0] if sign > 0 else [-0.11, -0.31, -10.0]
        cs[f"outside_{name}"] = case(q, lattice)
    # the wrap trap: A at the x-max end of row (y cell 0), B at the x-min end of the next row (y cell 1); the query beyond x-max must see A alone
    cs["wrap_trap"] = case([[1.6, 0.125, 0.125]], [[1.45, 0.125, 0.125], [0.05, 0.375, 0.125]])
    # ---- one heavy cell: 5 000 points inside a single cell, every other cell empty but for the two anchors'
    heavy = np.r_[anchors, rng.uniform(0.02, 0.23, size=(5000, 3))]
    cs["heavy_cell"] = case(np.r_[rng.uniform(0.0, 0.25, size=(24, 3)), rng.uniform(-0.3, 0.5, size=(12, 3)), [[3.0, 3.0, 3.0]]], heavy)
    # ---- coordinates: negative ones, points within 1e-6 of 0 on both sides (floor, not truncation), duplicates (the smallest index)
    tiny = np.array([[sx * 1e-7, sy * 3e-7, sz * 5e-7] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    cs["around_zero"] = case(np.r_[tiny * 1.5, box(40, -0.3, 0.3)], np.r_[box(100, -0.5, 0.5), tiny])
    base = box(24, -0.4, 0.4)
    dup = np.r_[base, base[[3, 3, 17, 5]], base[:2]]                  # records 24 .. 29 repeat 3, 3, 17, 5, 0, 1
    cs["dup_ref"] = case(np.r_[base[[3, 17, 5, 0, 1]], base[[3, 17]] + 1e-3, box(10, -0.4, 0.4)], dup[::-1].copy())   # reversed: the LATER copy is the original
    # exact ties that are no duplicates: sign flips of a component about the query, and 3-4-5 multiples of 2^-6 (squares and sums exact)
    u = 2.0 ** -6
    cs["exact_ties"] = case([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
                            [[3 * u, 4 * u, 0.0], [-3 * u, 4 * u, 0.0], [3 * u, -4 * u, 0.0], [5 * u, 0.0, 0.0], [0.0, 0.0, -5 * u],
                             [1.0 + 6 * u, 1.0, 1.0 + 8 * u], [1.0 - 6 * u, 1.0, 1.0 - 8 * u], [1.0, 1.0 + 10 * u, 1.0]])
    # d2 == max_dist^2 exactly is matched (3-4-5 at 5 * 2^-4), the next float outward is not; thr[0] sits on an exact tie too
    e = 2.0 ** -4
    out4 = np.nextafter(np.float32(4 * e), np.float32(np.inf))
    cs["reach_exact"] = case([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [20.0, 0.0, 0.0]],
                             [[3 * e, 4 * e, 0.0], [10.0 + 3 * e, out4, 0.0], [20.0, 1.5 * e, -2 * e]], max_dist=5 * e, thr=(2.5 * e, 5 * e))
    # ---- far-apart clusters: 3 km apart under max_dist 0.05 - 36 000 x 36 000 x 32 000 cells of 0.05 m, so the edge has to double
    far = np.array([1800.0, 1800.0, 1600.0])
    cl = np.r_[rng.uniform(0.0, 1.0, size=(64, 3)), far + rng.uniform(0.0, 1.0, size=(64, 3))]
    qf = np.r_[cl[[5, 70]] + 0.01, rng.uniform(0.0, 1.0, size=(20, 3)), far + rng.uniform(0.0, 1.0, size=(20, 3)), [far / 2]]
    cs["far_clusters"] = case(qf, cl, max_dist=0.05, thr=(0.01, 0.02, 0.03, 0.05))
    cs["one_cell"] = case(rng.uniform(0.1, 0.9, size=(30, 3)), rng.uniform(0.1, 0.9, size=(50, 3)), max_dist=10.0, thr=())
    # ---- a cloud against itself: every d2 exactly 0, j(i) = i but behind an earlier duplicate
    own = box(96)
    own[[40, 41]] = own[7]
    own[90] = own[40]
    cs["self"] = case(own, own)
    # ---- status: NaN / inf on either side, a coordinate at |p / max_dist| = 2^30 exactly, and the largest one that is still in range
    good_q, good_r = box(20), box(30)
    for name, side, value in (("nan_query", 0, np.nan), ("inf_query", 0, np.inf), ("nan_ref", 1, np.nan), ("inf_ref", 1, -np.inf)):
        q, r = good_q.copy(), good_r.copy()
        (q if side == 0 else r)[11, 1] = value
        cs[name] = case(q, r)
    md = 2.0 ** -10
    cs["range_query"] = case([[0.0, 0.0, 0.0], [0.0, -2.0 ** 20, 0.0]], [[0.0, 0.0, 0.0005]], max_dist=md, thr=(md,))
    cs["range_ref"] = case([[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0005], [2.0 ** 20, 0.0, 0.0]], max_dist=md, thr=(md,))
    inside = np.nextafter(np.float32(2.0 ** 20), np.float32(0.0))
    cs["range_edge_inside"] = case([[0.0, 0.0, 0.0], [inside, 0.0, 0.0005]], [[0.0, 0.0, 0.0005], [inside, 0.0, 0.0]], max_dist=md, thr=(md,))
    return cs


def load():
    """The frozen inputs of tests/golden/c2c_cases.npz, in the table's order."""
    z = np.load(GOLDEN)
    return {str(n): dict(query=z[f"{n}/in/query"], ref=z[f"{n}/in/ref"], max_dist=float(z[f"{n}/in/max_dist"][0]), thr=z[f"{n}/in/thr"]) for n in z["names"]}


def golden():
    """{case: dict(j, matched, rmse, mean, max, n_matched, n_within, worst, status)} of the frozen file."""
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = {k: z[f"{n}/out/{k}"] for k in ("j", "matched", "n_within")}
        g.update({k: float(z[f"{n}/out/{k}"][0]) for k in ("rmse", "mean", "max")})
        g.update({k: int(z[f"{n}/out/{k}"][0]) for k in ("n_matched", "worst", "status")})
        out[str(n)] = g
    return out


CASES = load() if os.path.exists(GOLDEN) else build()
NAMES = list(CASES)


def tol(c):
    return C * ULP * c["max_dist"]


def groups():
    """The cases that can share one call - equal max_dist and thresholds - as {(max_dist, thr bytes): [names]} in the table's order."""
    g = {}
    for n, c in CASES.items():
        g.setdefault((c["max_dist"], c["thr"].tobytes()), []).append(n)
    return g
