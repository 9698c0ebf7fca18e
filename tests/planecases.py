"""The frozen tables of the point-to-plane alignment cases (lk_clouds_align_plane_dev, lk_clouds_align_plane) and of the normals cases
(lk_clouds_normals_dev, lk_clouds_normals): seeded, listed by name, small.

An alignment case is tests/aligncases.py's dict with `normals` [m, 3] float32, one per reference point, as the generator gives them (the face's
axis; NaN where the case takes a plane away; scaled where it says so).  A normals case is a dict: cloud [n, 3] float32, radius, min_pts,
min_planarity.  build() / build_normals() are the seeded generators; the tables the tests use (CASES, NCASES) are their output as FROZEN in
tests/golden/plane_cases.npz, beside each case's expected values from the definitions run at 50 digits (tests/golden/make_plane_cases.py).  The
generator ASSERTS that every decision is clear by 2^10 times the tolerance below carried over to the quantity decided, or is an exact tie that
float64 ties too: every decision of the point-to-point table (nearest against runner-up, matched against the reach, both stop comparisons,
thresholds, worst), n_u >= 6 and `normal finite` (integers and bit patterns, clear once the matched flags are), every Cholesky pivot of the scaled
matrix either >= 2^-10 or zero at 50 digits, w against min_planarity, n_i against min_pts (membership of a neighbourhood by the margin on the
distance) and the component that gives the sign.  So counts, indices, iters, statuses and n_used are compared exactly.

TOLERANCE, following tests/aligncases.py.  With L the largest coordinate magnitude of the pair:
    |R_dev - R_50|_max <= C_R * 2^-53,    |t_dev - t_50|_max <= C_T * 2^-53 * L,    figures within C_FIG * 2^-53 * max_dist
(rmse_first, step_trans, the final rmse / mean / max and the two rmse_plane in metres - a plane residual is a distance times |n|, and the table's
normals have |n| <= 2 - step_rot in radians against the same number).  A normal: its angle to the 50-digit normal <= C_N * 2^-24, and
|w_dev - w_50| <= C_W * 2^-24 (the record is float32; half an ulp of a component is 2^-25).  Each C is 16 * max(1, worst ratio that
legkilo_amd.cloudmetrics reaches against the 50-digit values over this table).  Measured on this table:
    RATIO_R = 875.3, RATIO_T = 857.5, RATIO_FIG = 18610 - all three at "far": the residual e = n . (m - r) is formed from moved points at (3000, 2000,
        100), where one ulp of a coordinate is 2^-53 * 3000 m, and the solve divides it by the cloud's extent of 2 m: the rotation carries 2^-53 * L /
        extent whoever computes it.  (The point-to-point solve does not: it takes R from the ORIGINAL points about their centroids.)  Every case
        at the origin stays below 3, 1 and 20, which tests/test_plane_host.py asserts as well.
    RATIO_N = 0.53 ("tilted_50m"), RATIO_W = 0.5 ("n255"): the rounding to float32.
tests/test_plane_host.py re-measures them and fails if one exceeds twice its recorded value (or 1, where the recorded value is below 1).
EPS_TRANS is 1e-6 here (1e-3 for the far pair): with these C a step must keep 2e-8 m (3e-5 m at 3000 m) from eps_trans to be clear.
"""
import os

import numpy as np

import aligncases as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_cases.npz")
RATIO_R, RATIO_T, RATIO_FIG, RATIO_N, RATIO_W = 875.3, 857.5, 18610.0, 0.53, 0.5
C_R, C_T, C_FIG, C_N, C_W = (16.0 * max(1.0, v) for v in (RATIO_R, RATIO_T, RATIO_FIG, RATIO_N, RATIO_W))
ULP, ULP32 = 2.0 ** -53, 2.0 ** -24
NO_MATCH = 0xFFFFFFFF
FEW, CONVERGED, BAD_T0, DEGENERATE = 4, 8, 16, 32
M, THR, MAX_ITER, EPS_ROT, IDENTITY = ac.M, ac.THR, ac.MAX_ITER, ac.EPS_ROT, ac.IDENTITY
EPS_TRANS = 1e-6      # (aligncases has 1e-8; with this table's C_R and C_T a step has to stay 2e-8 m away from it to be clear, which 1e-8 cannot offer)
FIGURES = ac.FIGURES + ("rmse_plane_first", "rmse_plane")
SEED_BUMP = {}


def corner(rng, n=300, faces=(0, 1, 2)):
    """aligncases.corner with each point's face normal: a jittered lattice of spacing 0.2 m on the faces x = 0, y = 0, z = 0 (those of `faces`), 100
    points a face, in a seeded order -> (points [n, 3], normals [n, 3])."""
    k = np.arange(1, 11) * 0.2
    a, b = (v.reshape(-1) for v in np.meshgrid(k, k, indexing="ij"))
    pts, nrm = [], []
    for axis in faces:
        p, v = np.zeros((100, 3)), np.zeros((100, 3))
        p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a + rng.uniform(-0.03, 0.03, 100), b + rng.uniform(-0.03, 0.03, 100)
        v[:, axis] = 1.0
        pts.append(p), nrm.append(v)
    order = rng.permutation(100 * len(faces))[:n]
    return np.concatenate(pts)[order], np.concatenate(nrm)[order]


def case(query, ref, normals, **kw):
    kw.setdefault("eps_trans", EPS_TRANS)
    c = ac.case(query, ref, **kw)
    c["normals"] = np.ascontiguousarray(np.asarray(normals, dtype=np.float32).reshape(-1, 3))
    assert len(c["normals"]) == len(c["ref"])
    return c


def posed(master, nrm, rng, nq, nr, R, t):
    """(query, reference): the first nr master points, and the first nq of them taken back by the motion (R, t) about the master's centre after a
    seeded shift of up to 4 mm INSIDE each one's face (none along an axis its normal has a part in).  The shift leaves the plane residuals and the
    answer alone and gives the final search distances of millimetres that differ from point to point - so `worst` and the thresholds are clear by
    this table's margin, which residuals of float32 rounding alone (1e-7 m, a nanometre apart) would not be."""
    slid = master[:nq] + rng.uniform(-0.004, 0.004, (nq, 3)) * (nrm[:nq] == 0.0)
    return ac.inverse_apply(ac.about(R, np.asarray(t, dtype=np.float64), master.mean(0)), slid), master[:nr]


def two_a_face(master, nrm):
    """Indices of the first two points of each face in the master's order: six points that hold all six freedoms."""
    return np.sort(np.concatenate([np.flatnonzero(nrm[:, a] == 1.0)[:2] for a in range(3)]))


def build_case(name, bump=0):
    rng = np.random.default_rng([20261022, bump] + [ord(ch) for ch in name.replace("far_origin", "far")])
    S = ac.SMALL
    if name == "s0_0":
        return case(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), kind="status")
    if name in ("s6_65", "five_used"):                            # the smallest solve, and one used point fewer
        master, nrm = corner(rng)
        six = two_a_face(master[:65], nrm[:65])
        q, r = posed(master, nrm, rng, 65, 65, S["R"], S["t"])
        return case(q[six[:6 if name == "s6_65" else 5]], r, nrm[:65], kind="posed" if name == "s6_65" else "status")
    if name in ("s255_257", "s257_255"):
        nq, nr = (int(v) for v in name[1:].split("_"))
        master, nrm = corner(rng)
        q, r = posed(master, nrm, rng, nq, nr, S["R"], S["t"])
        return case(q, r, nrm[:nr])
    if name in ac.MOTIONS:
        master, nrm = corner(rng)
        q, r = posed(master, nrm, rng, 64, 65, *ac.MOTIONS[name])
        return case(q, r, nrm[:65])
    if name == "identity":
        master, nrm = corner(rng, 65)
        return case(master, master, nrm)
    if name == "t0_answer":
        master, nrm = corner(rng)
        q, r = posed(master, nrm, rng, 64, 65, S["R"], S["t"])
        return case(q, r, nrm[:65], T0=ac.about(S["R"], S["t"], master.mean(0)))
    if name in ("iter0", "iter1", "eps0"):
        master, nrm = corner(rng)
        R, t = (ac.rot(2, 4.0) @ ac.rot(0, -3.0), np.array([0.05, 0.04, -0.03])) if name == "eps0" else (S["R"], S["t"])
        q, r = posed(master, nrm, rng, 64, 65, R, t)
        return case(q, r, nrm[:65], max_iter={"iter0": 0, "iter1": 1, "eps0": 2}[name], eps_rot=0.0 if name == "eps0" else EPS_ROT,
                    eps_trans=0.0 if name == "eps0" else EPS_TRANS)
    if name in ("far", "far_origin"):                             # coordinates on a 2^-12 m raster: the same clouds at (3000, 2000, 100) are exact
        master, nrm = corner(rng)
        q, r = posed(master, nrm, rng, 64, 65, S["R"], S["t"])
        q, r = np.round(q * 4096.0) / 4096.0, np.round(r * 4096.0) / 4096.0
        o = np.array([3000.0, 2000.0, 100.0]) if name == "far" else 0.0
        return case(q + o, r + o, nrm[:65], eps_trans=1e-3)       # (at 3000 m the margin on a step is 3e-5 m: the steps are 3e-2, 2e-4 and 7e-9)
    if name == "plane":                                           # one face: in-plane shifts and the turn about its normal are unobserved - a zero diagonal
        master, nrm = corner(rng, 100, faces=(2,))
        q, r = posed(master, nrm, rng, 48, 100, ac.rot(0, 1.0), [0.0, 0.0, 0.01])
        return case(q, r, nrm, kind="status")
    if name == "parallel":                                        # two parallel walls (x = 0 and x = 2.2) and the floor: the shift along y is unobserved
        master, nrm = corner(rng, 200, faces=(0, 2))
        far_wall = (nrm[:, 0] == 1.0) & (np.arange(200) % 2 == 0)
        master[far_wall, 0] = 2.2
        q, r = posed(master, nrm, rng, 64, 200, ac.rot(1, 1.0), [0.01, 0.0, 0.01])
        return case(q, r, nrm, kind="status")
    if name == "parallel_diag":                                   # the same with the walls' normals (1, 1, 0): no zero diagonal - a zero pivot
        master, nrm = corner(rng, 200, faces=(0, 2))
        wall = nrm[:, 0] == 1.0
        far_wall = wall & (np.arange(200) % 2 == 0)
        master[wall, 0] = np.where(far_wall[wall], 2.2, 0.0) - master[wall, 1]      # the walls x + y = 0 and x + y = 2.2
        nrm[wall, 1] = 1.0
        q, r = posed(master, nrm, rng, 64, 200, ac.rot(2, 0.5), [0.005, 0.005, 0.01])
        return case(q, r, nrm, kind="status")
    if name == "nz0":                                             # two walls, no floor: every normal has nz == 0 - the diagonal entry of the shift along z is 0
        master, nrm = corner(rng, 200, faces=(0, 1))
        q, r = posed(master, nrm, rng, 64, 200, ac.rot(2, 1.0), [0.01, 0.01, 0.0])
        return case(q, r, nrm, kind="status")
    if name in ("third_nan", "all_nan"):
        master, nrm = corner(rng)
        q, r = posed(master, nrm, rng, 64, 65, S["R"], S["t"])
        nrm = nrm[:65].copy()
        sel = np.arange(65) % 3 == 1 if name == "third_nan" else np.ones(65, dtype=bool)
        nrm[sel, rng.integers(0, 3, int(sel.sum()))] = np.nan     # one component is enough
        return case(q, r, nrm, kind="posed" if name == "third_nan" else "status")
    if name == "nonunit":                                         # a length per face: 2^-14, 2, 1/2 - without the scaling a pivot is 2^-28 * n_u
        master, nrm = corner(rng)
        q, r = posed(master, nrm, rng, 64, 65, S["R"], S["t"])
        return case(q, r, nrm[:65] * np.array([2.0 ** -14, 2.0, 0.5]))
    if name in ("nan_query", "nan_ref", "range_query", "bad_t0"):
        master, nrm = corner(rng)
        q, r = posed(master, nrm, rng, 20, 30, S["R"], S["t"])
        T0 = None
        if name == "nan_query":
            q[11, 1] = np.nan
        elif name == "nan_ref":
            r = r.copy()
            r[7, 2] = np.nan
        elif name == "range_query":
            q[3, 0] = 3.0e8
        else:
            T0 = IDENTITY.copy()
            T0[10] = np.nan
        return case(q, r, nrm[:30], T0=T0, kind="status")
    raise KeyError(name)


ORDER = ["s0_0", "s6_65", "trans", "rot_x", "five_used", "rot_y", "rot_z", "both", "identity", "t0_answer", "s255_257", "s257_255", "far_origin", "far", "plane",
         "parallel", "parallel_diag", "nz0", "third_nan", "all_nan", "nonunit", "nan_query", "nan_ref", "range_query", "bad_t0", "iter0", "iter1", "eps0"]


def build():
    return {n: build_case(n, SEED_BUMP.get(n, 0)) for n in ORDER}


# ---- the normals cases
N_RADIUS, N_MIN_PTS, N_MIN_PLAN = 0.45, 5, 0.3


def ncase(cloud, radius=N_RADIUS, min_pts=N_MIN_PTS, min_planarity=N_MIN_PLAN):
    return dict(cloud=np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 3)), radius=float(radius), min_pts=int(min_pts),
                min_planarity=float(min_planarity))


def lattice(rng, n=8, jitter=0.03):
    k = np.arange(1, n + 1) * 0.2
    a, b = (v.reshape(-1) for v in np.meshgrid(k, k, indexing="ij"))
    return a + rng.uniform(-jitter, jitter, n * n), b + rng.uniform(-jitter, jitter, n * n)


def build_ncase(name, bump=0):
    rng = np.random.default_rng([20261023, bump] + [ord(ch) for ch in name])
    if name == "plane":                                           # z exactly 0: l0 = 0
        a, b = lattice(rng)
        return ncase(np.stack([a, b, np.zeros(64)], axis=1))
    if name == "tilted_50m":                                      # a wall tilted about two axes, 50 m out: l0 is the float32 storage's noise
        a, b = lattice(rng)
        p = np.stack([a, b, np.zeros(64)], axis=1) @ (ac.rot(0, 31.0) @ ac.rot(1, -17.0)).T + np.array([40.0, -30.0, 3.0])
        return ncase(p)
    if name == "edge":                                            # two faces: near the edge the planarity falls below the threshold
        p, _ = corner(rng, 200, faces=(0, 1))
        return ncase(p)
    if name == "corner":
        p, _ = corner(rng, 300)
        return ncase(p)
    if name == "line":                                            # every point on the x axis, exactly: l0 = l1 = 0, w = 0
        x = np.arange(1, 41) * 0.1 + rng.uniform(-0.02, 0.02, 40)
        return ncase(np.stack([x, np.zeros(40), np.zeros(40)], axis=1))
    if name == "duplicates":                                      # twelve copies of one point (l2 = 0: w = 0) beside a small plane, some of its points doubled
        a, b = lattice(rng, 5)
        pl = np.stack([a, b, np.zeros(25)], axis=1)
        return ncase(np.concatenate([np.tile([[5.0, 5.0, 5.0]], (12, 1)), pl, pl[::3]]))
    if name in ("at_min_pts", "below_min_pts"):                   # a 3 x 3 patch of spacing 0.1: every point sees all nine - min_pts 9 and 10
        a, b = (v.reshape(-1) for v in np.meshgrid(np.arange(3) * 0.1, np.arange(3) * 0.1, indexing="ij"))
        p = np.stack([a + rng.uniform(-0.01, 0.01, 9), b + rng.uniform(-0.01, 0.01, 9), np.zeros(9)], axis=1)
        return ncase(p, min_pts=9 if name == "at_min_pts" else 10)
    if name in ("w_above", "w_below"):                            # a strip 5 long and 2 deep, every point seeing all ten: w = l1 / l2 near 0.1 - the threshold on either side of it
        a, b = (v.reshape(-1) for v in np.meshgrid(np.arange(5) * 0.1, np.arange(2) * 0.1, indexing="ij"))
        p = np.stack([a + rng.uniform(-0.01, 0.01, 10), b + rng.uniform(-0.01, 0.01, 10), np.zeros(10)], axis=1)
        return ncase(p, radius=1.0, min_pts=3, min_planarity=0.02 if name == "w_above" else 0.5)
    if name.startswith("n") and name[1:].isdigit():               # clouds of 0, 1, 255 and 257 points: a plane in a seeded order
        n = int(name[1:])
        a, b = lattice(rng, 17)
        return ncase(rng.permutation(np.stack([a, b, np.zeros(289)], axis=1))[:n])
    if name in ("nan", "range"):
        a, b = lattice(rng, 5)
        p = np.stack([a, b, np.zeros(25)], axis=1)
        p[7, 1] = np.nan if name == "nan" else 6.0e8
        return ncase(p)
    raise KeyError(name)


def sign_tie():
    """NOT a case of the table - its sign decision lies below the table's margin on purpose: four points of the plane through (-2^24, -2^24, .) and
    (2^24, 2^24 - 1, .), whose normal is (-(2^25 - 1), 2^25, 0) / |.|.  In float64 the second component is the larger by 2.1e-8 (the closed form is
    good to 1e-15) and is made positive; rounded to float32 the two tie, and a sign rule applied after the rounding takes the first and flips the
    normal."""
    N = 2.0 ** 24
    return ncase([[-N, -N, 0.0], [-N, -N, 1e7], [N, N - 1.0, 0.0], [N, N - 1.0, 1e7]], radius=1e9, min_pts=3, min_planarity=0.0)


NORDER = ["plane", "tilted_50m", "edge", "n0", "corner", "line", "n1", "duplicates", "at_min_pts", "below_min_pts", "nan", "w_above", "w_below", "n255", "range", "n257"]
NSEED_BUMP = {}


def build_normals():
    return {n: build_ncase(n, NSEED_BUMP.get(n, 0)) for n in NORDER}


# ---- the frozen file
OUT_ARRAYS = ("T", "j_first", "matched_first", "j", "matched", "n_within", "pivots")
OUT_FLOATS = ac.OUT_FLOATS + ("rmse_plane_first", "rmse_plane")
OUT_INTS = ac.OUT_INTS + ("n_used_first", "n_used")
N_OUT = ("n", "w", "valid", "dense", "vec", "status")


def load():
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = lambda k: z[f"{n}/in/{k}"]   # noqa: E731
        out[str(n)] = dict(query=g("query"), ref=g("ref"), normals=g("normals"), max_dist=float(g("max_dist")[0]), thr=g("thr"), has_T0=bool(g("has_T0")[0]), T0=g("T0"),
                           max_iter=int(g("max_iter")[0]), eps_rot=float(g("eps_rot")[0]), eps_trans=float(g("eps_trans")[0]), kind=str(g("kind")[0]))
    return out


def load_normals():
    z = np.load(GOLDEN)
    return {str(n): dict(cloud=z[f"N/{n}/in/cloud"], radius=float(z[f"N/{n}/in/radius"][0]), min_pts=int(z[f"N/{n}/in/min_pts"][0]),
                         min_planarity=float(z[f"N/{n}/in/min_planarity"][0])) for n in z["nnames"]}


def golden():
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = {k: z[f"{n}/out/{k}"] for k in OUT_ARRAYS}
        g.update({k: float(z[f"{n}/out/{k}"][0]) for k in OUT_FLOATS})
        g.update({k: int(z[f"{n}/out/{k}"][0]) for k in OUT_INTS})
        out[str(n)] = g
    return out


def golden_normals():
    z = np.load(GOLDEN)
    return {str(n): {k: z[f"N/{n}/out/{k}"] for k in N_OUT} for n in z["nnames"]}


CASES = load() if os.path.exists(GOLDEN) else build()
NCASES = load_normals() if os.path.exists(GOLDEN) else build_normals()
NAMES, NNAMES = list(CASES), list(NCASES)
extent = ac.extent


def groups():
    """The alignment cases that can share one call - equal scalar arguments - as {key: [names]} in the table's order."""
    g = {}
    for n, c in CASES.items():
        g.setdefault((c["max_dist"], c["thr"].tobytes(), c["max_iter"], c["eps_rot"], c["eps_trans"]), []).append(n)
    return g


def ngroups():
    g = {}
    for n, c in NCASES.items():
        g.setdefault((c["radius"], c["min_pts"], c["min_planarity"]), []).append(n)
    return g


def compare(name, got, want, c=None):
    """One alignment result against the golden values.  got: aligncases.compare's dict and rmse_plane_first, rmse_plane, n_used_first, n_used.
    Decisions exactly, T and the figures within tolerance.  Returns the ratios reached: dict(R=, T=, FIG=)."""
    c = CASES[name] if c is None else c
    L, md = extent(c), c["max_dist"]
    T = np.asarray(got["T"], dtype=np.float64).reshape(12)
    ratios = dict(R=0.0, T=0.0, FIG=0.0)
    assert (int(got["iters"]), int(got["status"])) == (want["iters"], want["status"]), (name, int(got["iters"]), int(got["status"]), want["iters"], want["status"])
    assert (int(got["n_matched_first"]), int(got["n_matched"]), int(got["worst"])) == (want["n_matched_first"], want["n_matched"], want["worst"]), name
    assert (int(got["n_used_first"]), int(got["n_used"])) == (want["n_used_first"], want["n_used"]), (name, int(got["n_used_first"]), int(got["n_used"]))
    assert list(got["n_within"])[:len(c["thr"])] == want["n_within"].tolist(), name
    for k in ("j_first", "matched_first", "j", "matched"):
        if k in got and got[k] is not None:
            assert np.array_equal(np.asarray(got[k]), want[k]), (name, k)
    if want["iters"] == 0:
        assert T.tobytes() == c["T0"].tobytes(), (name, "T0 is copied through: no solve was taken")
    else:
        ratios["R"] = float(np.abs(T[:9] - want["T"][:9]).max() / ULP)
        ratios["T"] = float(np.abs(T[9:] - want["T"][9:]).max() / (ULP * L))
        assert ratios["R"] <= C_R and ratios["T"] <= C_T, (name, ratios)
        assert ac.is_rotation(T[:9]), name
    for f in FIGURES:
        assert np.isnan(got[f]) == np.isnan(want[f]), (name, f, got[f], want[f])
        if not np.isnan(want[f]):
            ratio = abs(float(got[f]) - want[f]) / (ULP * md)
            assert ratio <= C_FIG, (name, f, ratio, float(got[f]), want[f])
            ratios["FIG"] = max(ratios["FIG"], ratio)
    return ratios


def angle(a, b):
    """The angle between two directions [.., 3] in the atan2 form (exact near 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(axis=-1))


def compare_normals(name, rec, n, want, n_valid=None, status=None):
    """One cloud's records float32 [m, 4] (and n_i where the caller has them) against the golden values: validity, density and n_i exactly, a valid
    normal by its angle, a dense point's w by its difference.  Returns dict(N=, W=): the ratios reached."""
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, 4)
    valid, dense = want["valid"].astype(bool), want["dense"].astype(bool)
    ratios = dict(N=0.0, W=0.0)
    if status is not None:
        assert int(status) == int(want["status"][0]), (name, status)
    if n_valid is not None:
        assert int(n_valid) == int(valid.sum()), (name, n_valid, int(valid.sum()))
    if n is not None and not int(want["status"][0]):
        assert np.array_equal(np.asarray(n), want["n"]), (name, "n_i")
    assert np.array_equal(~np.isnan(rec[:, 0]), valid) and np.array_equal(~np.isnan(rec[:, 3]), dense), (name, "validity")
    assert np.array_equal(np.isnan(rec[:, :3]).any(axis=1), np.isnan(rec[:, :3]).all(axis=1)), name
    if valid.any():
        ratios["N"] = float(angle(rec[valid, :3], want["vec"][valid]).max() / ULP32)
        assert ratios["N"] <= C_N, (name, ratios)
        assert np.abs(np.linalg.norm(rec[valid, :3].astype(np.float64), axis=1) - 1.0).max() <= 4.0 * ULP32, (name, "unit length")
        lead = np.argmax(np.abs(want["vec"][valid]), axis=1)
        assert (rec[valid, :3][np.arange(int(valid.sum())), lead] > 0).all(), (name, "sign")
    if dense.any():
        ratios["W"] = float(np.abs(rec[dense, 3].astype(np.float64) - want["w"][dense]).max() / ULP32)
        assert ratios["W"] <= C_W, (name, ratios)
    return ratios
