"""The frozen table of rigid-alignment cases (lk_clouds_align_dev, lk_clouds_align): seeded, listed by name, small.

A case is a dict: query [n, 3], ref [m, 3] (float32), max_dist, thr, T0 (12 float64, R row-major then t; the identity where the case gives none - the
entry takes NULL for it, has_T0 says which), max_iter, eps_rot, eps_trans and kind: "posed" (T is compared), "free" (degenerate geometry: only
what does not depend on a free direction is compared) or "status".  build() is the seeded generator; the table the tests use (CASES) is its output as
FROZEN in tests/golden/align_cases.npz, beside each case's expected values from the definition run at 50 digits (tests/golden/make_align_cases.py):
T, iters, status, the matched flags and j(i) of the first and of the final search, the figures.  The generator ASSERTS that every decision of every
iteration - nearest against runner-up, matched against the reach, n >= 3, both stop comparisons, thresholds, worst - is clear by 2^10 times the
tolerance below carried over to the quantity decided, or is an exact tie whose float64 values tie too; so counts, indices, iters and statuses are
compared exactly.  It also asserts for the posed cases that Horn's largest eigenvalue is separated from the next by a tenth of the spread in every
solve.  A case that fails an assertion is reseeded (SEED_BUMP), not excused.

TOLERANCE, following tests/c2ccases.py.  With L the largest coordinate magnitude of the pair:
    |R_dev - R_50|_max <= C_R * 2^-53,    |t_dev - t_50|_max <= C_T * 2^-53 * L,    figures within C_FIG * 2^-53 * max_dist
(rmse_first, step_trans and the final rmse / mean / max in metres, step_rot in radians against the same number).  Each C is 16 * max(1, worst ratio
that legkilo_amd.cloudmetrics.align reaches against the 50-digit values over this table): the factor 16 covers another summation order and
another eigen-solver.  Measured on this table:
    RATIO_R = 2.25      ("s257_255")
    RATIO_T = 2.82      ("far")
    RATIO_FIG = 12256.0 ("far": the clouds lie at (3000, 2000, 100), so one ulp of a moved coordinate is 2^-53 * 3000 m - 12 000 of these units of
                         2^-53 * max_dist, whoever computes it; every case at the origin stays below 20)
tests/test_align_host.py re-measures the three and fails if one exceeds twice its recorded value.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_cases.npz")
RATIO_R, RATIO_T, RATIO_FIG = 2.25, 2.82, 12256.0
C_R, C_T, C_FIG = (16.0 * max(1.0, v) for v in (RATIO_R, RATIO_T, RATIO_FIG))
ULP = 2.0 ** -53
NO_MATCH = 0xFFFFFFFF
FEW, CONVERGED, BAD_T0 = 4, 8, 16

M = 0.25
THR = (0.05, 0.125, 0.25)
MAX_ITER, EPS_ROT, EPS_TRANS = 30, 1e-6, 1e-8       # of most cases, so that they go into one call as many pairs
SIZES = [(0, 0), (0, 65), (65, 0), (1, 1), (2, 65), (3, 65), (63, 64), (64, 65), (255, 257), (256, 256), (257, 255)]   # (query, reference)
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
FIGURES = ("rmse_first", "step_rot", "step_trans", "rmse", "mean", "max")
# case name -> how often its seed was moved on after an assertion of the generator failed ("s3_65", seed 0: three nearly collinear points, Horn gap 0.05)
SEED_BUMP = {"s3_65": 1}


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def about(R, t, centre):
    """The 12 doubles of r = R (q - centre) + centre + t."""
    return np.r_[np.asarray(R).reshape(9), centre + t - R @ centre]


def inverse_apply(T, pts):
    R, t = T[:9].reshape(3, 3), T[9:]
    return (pts - t) @ R      # R^T (p - t), row-wise


def corner(rng, n=300):
    """A jittered lattice of spacing 0.2 m on three mutually perpendicular faces (an open corner), 100 points a face, in a seeded order.  The jitter
    is in the face's own plane: a point of the face z = 0 has z exactly 0."""
    k = np.arange(1, 11) * 0.2
    a, b = (v.reshape(-1) for v in np.meshgrid(k, k, indexing="ij"))
    faces = []
    for axis in range(3):
        p = np.zeros((100, 3))
        p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a + rng.uniform(-0.03, 0.03, 100), b + rng.uniform(-0.03, 0.03, 100)
        faces.append(p)
    return rng.permutation(np.concatenate(faces))[:n]


def case(query, ref, T0=None, max_iter=MAX_ITER, eps_rot=EPS_ROT, eps_trans=EPS_TRANS, max_dist=M, thr=THR, kind="posed"):
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))   # noqa: E731
    return dict(query=f(query), ref=f(ref), max_dist=float(max_dist), thr=np.asarray(thr, dtype=np.float64).reshape(-1), has_T0=T0 is not None,
                T0=IDENTITY.copy() if T0 is None else np.asarray(T0, dtype=np.float64).reshape(12).copy(), max_iter=int(max_iter), eps_rot=float(eps_rot),
                eps_trans=float(eps_trans), kind=kind)


SMALL = dict(R=rot(0, 1.1) @ rot(1, -0.9) @ rot(2, 1.3), t=np.array([0.021, -0.017, 0.013]))    # "a few centimetres and about 2 degrees"
MOTIONS = dict(trans=(np.eye(3), [0.03, -0.02, 0.025]), rot_x=(rot(0, 2.0), [0, 0, 0]), rot_y=(rot(1, -2.0), [0, 0, 0]), rot_z=(rot(2, 2.0), [0, 0, 0]),
               both=(SMALL["R"], SMALL["t"]))


def build_case(name, bump=0):
    rng = np.random.default_rng([20261021, bump] + [ord(ch) for ch in name.replace("far_origin", "far")])   # ("far" is "far_origin" moved: one seed)
    posed = lambda master, nq, nr, R, t: (inverse_apply(about(R, np.asarray(t, dtype=np.float64), master.mean(0)), master[:nq]), master[:nr])   # noqa: E731
    if name.startswith("s") and name[1].isdigit():
        nq, nr = (int(v) for v in name[1:].split("_"))
        master = corner(rng)
        q, r = posed(master, nq, nr, SMALL["R"], SMALL["t"])
        return case(q, r, kind="posed" if nq >= 3 and nr >= 3 else "status")
    if name in MOTIONS:
        return case(*posed(corner(rng), 64, 65, *MOTIONS[name]))
    if name == "identity":
        master = corner(rng, 65)
        return case(master, master)
    if name == "t0_answer":                                      # T0 is the motion the query was made with: one solve, and it moves by rounding only
        master = corner(rng)
        T = about(SMALL["R"], SMALL["t"], master.mean(0))
        return case(inverse_apply(T, master[:64]), master[:65], T0=T)
    if name in ("wide", "iter0", "iter0_t0", "iter1", "iter1_t0", "eps0", "eps0_t0"):
        master = corner(rng)
        R, t = (rot(2, 4.0) @ rot(0, -3.0), np.array([0.05, 0.04, -0.03])) if name.startswith("eps0") or name == "wide" else (SMALL["R"], SMALL["t"])
        q, r = posed(master, 64, 65, R, t)
        T0 = about(rot(1, 0.4), np.array([0.004, 0.0, -0.003]), master.mean(0)) if name.endswith("_t0") else None
        return case(q, r, T0=T0, max_iter={"wide": MAX_ITER, "iter0": 0, "iter1": 1, "eps0": 2}[name.split("_")[0]], eps_rot=0.0 if name.startswith("eps0") else EPS_ROT,
                    eps_trans=0.0 if name.startswith("eps0") else EPS_TRANS)
    if name in ("far", "far_origin"):                            # coordinates on a 2^-12 m raster: the same clouds at (3000, 2000, 100) are exact
        master = corner(rng)
        q, r = posed(master, 64, 65, SMALL["R"], SMALL["t"])
        q, r = np.round(q * 4096.0) / 4096.0, np.round(r * 4096.0) / 4096.0
        o = np.array([3000.0, 2000.0, 100.0]) if name == "far" else 0.0
        return case(q + o, r + o)
    if name == "mirror":                                         # a slab |z| <= 0.05 against its mirror image in z: the best orthogonal map is a reflection
        k = np.arange(1, 9) * 0.2
        a, b = (v.reshape(-1) for v in np.meshgrid(k, k, indexing="ij"))
        slab = np.stack([a + rng.uniform(-0.03, 0.03, 64), b + rng.uniform(-0.03, 0.03, 64), rng.uniform(-0.05, 0.05, 64)], axis=1)
        T = about(rot(2, 1.0), np.array([0.01, -0.01, 0.0]), slab.mean(0))
        return case(inverse_apply(T, slab), slab * [1.0, 1.0, -1.0])
    if name == "guard_t0":                                       # T0 shears x by 1e20 z: only the points with z == 0 stay inside the range guard
        master = corner(rng, 130)
        T0 = IDENTITY.copy()
        T0[2], T0[9:] = 1e20, [0.01, 0.015, 0.0]
        return case(master[:64], master[:65], T0=T0)
    if name == "partial":                                        # sixteen query points that have no partner: the centroids are of the matched ones only
        master = corner(rng)
        q, r = posed(master, 64, 65, SMALL["R"], SMALL["t"])
        return case(np.r_[q[:30], rng.uniform(4.0, 5.0, (16, 3)), q[30:]], r)
    if name in ("nan_query", "nan_ref", "range_query", "bad_t0"):
        master = corner(rng)
        q, r = posed(master, 20, 30, SMALL["R"], SMALL["t"])
        T0 = None
        if name == "nan_query":
            q[11, 1] = np.nan
        elif name == "nan_ref":
            r[7, 2] = np.nan
        elif name == "range_query":
            q[3, 0] = 3.0e8                                      # |p / max_dist| >= 2^30 from 2.7e8 on
        else:
            T0 = IDENTITY.copy()
            T0[10] = np.nan
        return case(q, r, T0=T0, kind="status")
    if name == "plane":                                          # one face only: sliding along it is held by the jitter alone
        k = np.arange(1, 9) * 0.2
        a, b = (v.reshape(-1) for v in np.meshgrid(k, k, indexing="ij"))
        face = np.stack([a + rng.uniform(-0.03, 0.03, 64), b + rng.uniform(-0.03, 0.03, 64), np.zeros(64)], axis=1)
        T = about(rot(2, 1.5), np.array([0.02, -0.01, 0.01]), face.mean(0))
        return case(inverse_apply(T, face[:48]), face, kind="free")
    if name == "line":                                           # every point on the x axis, exactly: the rotation about it is free
        x = np.arange(1, 41) * 0.2 + rng.uniform(-0.03, 0.03, 40)
        pts = np.stack([x, np.zeros(40), np.zeros(40)], axis=1)
        T0 = IDENTITY.copy()
        T0[9:] = [0.03, 0.02, -0.01]
        return case(pts[:32], pts, T0=T0, kind="free")
    raise KeyError(name)


ORDER = ([f"s{a}_{b}" for a, b in SIZES[:4]] + ["trans", "rot_x", "s2_65", "rot_y", "rot_z", "both", "identity", "s3_65", "t0_answer"]
         + [f"s{a}_{b}" for a, b in SIZES[6:]] + ["wide", "far_origin", "far", "mirror", "guard_t0", "partial", "nan_query", "nan_ref", "range_query", "bad_t0", "plane",
                                                  "line", "iter0", "iter0_t0", "iter1", "iter1_t0", "eps0", "eps0_t0"])


def build():
    return {n: build_case(n, SEED_BUMP.get(n, 0)) for n in ORDER}


IN_KEYS = ("query", "ref", "max_dist", "thr", "has_T0", "T0", "max_iter", "eps_rot", "eps_trans", "kind")
OUT_ARRAYS = ("T", "j_first", "matched_first", "j", "matched", "n_within")
OUT_FLOATS = ("rmse_first", "step_rot", "step_trans", "rmse", "mean", "max", "gap")
OUT_INTS = ("iters", "status", "n_matched_first", "n_matched", "worst", "clear", "c2c_tie")


def load():
    """The frozen inputs of tests/golden/align_cases.npz, in the table's order."""
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = lambda k: z[f"{n}/in/{k}"]   # noqa: E731
        out[str(n)] = dict(query=g("query"), ref=g("ref"), max_dist=float(g("max_dist")[0]), thr=g("thr"), has_T0=bool(g("has_T0")[0]), T0=g("T0"),
                           max_iter=int(g("max_iter")[0]), eps_rot=float(g("eps_rot")[0]), eps_trans=float(g("eps_trans")[0]), kind=str(g("kind")[0]))
    return out


def golden():
    """{case: dict of OUT_ARRAYS, OUT_FLOATS, OUT_INTS} of the frozen file."""
    z = np.load(GOLDEN)
    out = {}
    for n in z["names"]:
        g = {k: z[f"{n}/out/{k}"] for k in OUT_ARRAYS}
        g.update({k: float(z[f"{n}/out/{k}"][0]) for k in OUT_FLOATS})
        g.update({k: int(z[f"{n}/out/{k}"][0]) for k in OUT_INTS})
        out[str(n)] = g
    return out


CASES = load() if os.path.exists(GOLDEN) else build()
NAMES = list(CASES)


def extent(c):
    """L: the largest finite coordinate magnitude of the pair (1 for a pair without one)."""
    v = np.concatenate([c["query"].reshape(-1), c["ref"].reshape(-1)]).astype(np.float64)
    v = np.abs(v[np.isfinite(v)])
    return float(v.max()) if len(v) and v.max() > 0 else 1.0


def groups():
    """The cases that can share one call - equal scalar arguments - as {key: [names]} in the table's order."""
    g = {}
    for n, c in CASES.items():
        g.setdefault((c["max_dist"], c["thr"].tobytes(), c["max_iter"], c["eps_rot"], c["eps_trans"]), []).append(n)
    return g


def is_rotation(R, slack=64.0):
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    return np.abs(R @ R.T - np.eye(3)).max() <= slack * ULP and abs(np.linalg.det(R) - 1.0) <= slack * ULP


def compare(name, got, want, c=None):
    """One result against the golden values.  got: dict with T [12], iters, status, n_matched_first, rmse_first, step_rot, step_trans, rmse, mean,
    max, n_matched, n_within, worst and, where the caller has them, j_first / matched_first / j / matched.  Decisions exactly, T and the figures
    within tolerance, as the case's kind allows.  Returns the ratios reached: dict(R=, T=, FIG=) (0 where nothing was measured)."""
    c = CASES[name] if c is None else c
    L, md = extent(c), c["max_dist"]
    T = np.asarray(got["T"], dtype=np.float64).reshape(12)
    ratios = dict(R=0.0, T=0.0, FIG=0.0)
    if c["kind"] == "status" and want["status"] & (1 | 2 | BAD_T0):
        assert T.tobytes() == c["T0"].tobytes(), (name, "T0 is copied through")
    if c["kind"] == "free" and not want["clear"]:                # a free direction decided a stop comparison: only what holds whatever it was
        assert is_rotation(T[:9]), name
        assert np.isnan(got["rmse"]) or got["rmse"] <= got["rmse_first"] + C_FIG * ULP * md, name
        return ratios
    assert (int(got["iters"]), int(got["status"])) == (want["iters"], want["status"]), (name, int(got["iters"]), int(got["status"]), want["iters"], want["status"])
    assert (int(got["n_matched_first"]), int(got["n_matched"]), int(got["worst"])) == (want["n_matched_first"], want["n_matched"], want["worst"]), name
    assert list(got["n_within"])[:len(c["thr"])] == want["n_within"].tolist(), name
    for k in ("j_first", "matched_first", "j", "matched"):
        if k in got and got[k] is not None:
            assert np.array_equal(np.asarray(got[k]), want[k]), (name, k)
    if c["kind"] == "free":
        assert is_rotation(T[:9]), name
        assert np.isnan(got["rmse"]) or got["rmse"] <= got["rmse_first"] + C_FIG * ULP * md, name
    elif not (want["status"] & (1 | 2 | BAD_T0)):
        ratios["R"] = float(np.abs(T[:9] - want["T"][:9]).max() / ULP)
        ratios["T"] = float(np.abs(T[9:] - want["T"][9:]).max() / (ULP * L))
        assert ratios["R"] <= C_R and ratios["T"] <= C_T, (name, ratios)
        if want["iters"]:
            assert is_rotation(T[:9]), name
    for f in FIGURES:
        assert np.isnan(got[f]) == np.isnan(want[f]), (name, f, got[f], want[f])
        if not np.isnan(want[f]):
            if want[f] == 0.0 and f.startswith("step"):
                assert got[f] == 0.0, (name, f, "an exact tie of the stop comparison: the float64 value ties too")
            ratio = abs(float(got[f]) - want[f]) / (ULP * md)
            assert ratio <= C_FIG, (name, f, ratio, float(got[f]), want[f])
            ratios["FIG"] = max(ratios["FIG"], ratio)
    return ratios
