"""Writes tests/golden/planecloud_cases.npz: the inputs of tests/planecloudcases.py::build() as float32 and, per case, what lk_clouds_planes_dev has to give.

    python tests/golden/make_planecloud_cases.py [path]

Decisions are taken in EXACT integer arithmetic: a float32 coordinate is an integer multiple of 2^-k, so with every coordinate of a cloud scaled by
one power of two every u x v, q and s is a Python integer (numpy arrays of objects), and with dist and the axis as exact fractions s*s <= dist^2 q
and g*g < cos^2 q aa are comparisons of integers.  The sampler is planecloudcases.sample, in Python integers.  evaluate() ASSERTS what lets the tests
compare every whole number exactly - see tests/planecloudcases.py for the list - and that the cases with an exact tie are the ones named there.
The coefficients of every plane come from mpmath at 50 digits: centroid, covariance / n, mpmath.eigsy; the generator decides there whether a refit's
normal is conditioned (eig[1] - eig[0] above GAP_FRACTION of eig[2])."""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import planecloudcases as pc  # noqa: E402

MARGIN = 2 ** 40
mpmath.mp.dps = 50


def status_of(c):
    v = c["cloud"].astype(np.float64)
    fin = np.isfinite(v)
    return (0 if fin.all() else 1) | (2 if (np.abs(v[fin]) >= 2.0 ** 30).any() else 0)


def scaled_ints(cloud):
    """(P, S): the cloud as an object array of Python integers, P = cloud * S exactly, S a power of two."""
    den = 1
    for v in cloud.reshape(-1):
        den = max(den, float(v).as_integer_ratio()[1])
    return np.array([[int(Fraction(float(v)) * den) for v in row] for row in cloud], dtype=object).reshape(len(cloud), 3), den


def clear(lhs, rhs, what):
    """lhs against rhs, elementwise on object arrays of integers: equal, or apart by a relative 2^-40 -> the mask of exact ties"""
    tie = lhs == rhs
    far = np.abs(lhs - rhs) * MARGIN >= np.abs(rhs)
    assert (tie | far).all(), what
    return tie.astype(bool)


def exact_round(name, P, S, idx, c, ties):
    """One round on the remainder P [m, 3] (integers) with the sampled positions idx [H, 3] -> inside bool [H, m] (all False for a skipped
    hypothesis), from integers alone.  S: the power of two the coordinates were scaled by - s*s carries S^6, q S^4."""
    d2 = Fraction(c["dist"]) * Fraction(c["dist"]) * S * S   # the exact square; the rounded product differs by 2^-53, inside the margin
    a, u, v = P[idx[:, 0]], P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]]
    mv = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    q = mv[:, 0] * mv[:, 0] + mv[:, 1] * mv[:, 1] + mv[:, 2] * mv[:, 2]
    ok = (q > 0).astype(bool)
    if c["axis"] is not None:
        ax = [Fraction(v_) for v_ in c["axis"]]
        den = max(f.denominator for f in ax)
        an = [int(f * den) for f in ax]                                         # the axis times den: g and aa scale alike
        g = mv[:, 0] * an[0] + mv[:, 1] * an[1] + mv[:, 2] * an[2]
        aa = an[0] * an[0] + an[1] * an[1] + an[2] * an[2]
        c2 = Fraction(c["cos_max_angle"]) * Fraction(c["cos_max_angle"])
        lhs, rhs = g * g * c2.denominator, q * (c2.numerator * aa)
        tie = clear(lhs[ok], rhs[ok], (name, "the axis test is neither clear nor an exact tie"))
        if tie.any():
            assert float(c["cos_max_angle"]) ** 2 == c2, (name, "an exact tie of the axis test under an inexact square")
            ties["axis"].add(name)
        ok &= ~(lhs < rhs).astype(bool)
    inside = np.zeros((len(idx), len(P)), dtype=bool)
    for h in np.flatnonzero(ok):
        e = P - a[h]
        s = e[:, 0] * mv[h, 0] + e[:, 1] * mv[h, 1] + e[:, 2] * mv[h, 2]
        lhs, rhs = s * s * d2.denominator, np.full(len(P), q[h] * d2.numerator, dtype=object)
        if clear(lhs, rhs, (name, int(h), "membership neither clear nor an exact tie")).any():
            assert float(c["dist"]) * float(c["dist"]) * S * S == d2, (name, "an exact tie under an inexact dist * dist")
            ties["threshold"].add(name)
        inside[h] = (lhs <= rhs).astype(bool)
    return inside


def refit(points, axis):
    """50-digit coefficients of one plane from its inliers (float64 rows, exact images of the float32 coordinates)"""
    mp = mpmath.mp
    n = len(points)
    rows = [[mp.mpf(float(v)) for v in p] for p in points]
    cen = [mp.fsum(r[k] for r in rows) / n for k in range(3)]
    A = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            A[i, j] = mp.fsum((r[i] - cen[i]) * (r[j] - cen[j]) for r in rows) / n
    E, Q = mp.eigsy(A)
    order = sorted(range(3), key=lambda k: E[k])
    eig = [E[k] for k in order]
    nrm = [Q[i, order[0]] for i in range(3)]
    if axis is not None:
        flip = not (mp.fsum(nrm[k] * mp.mpf(axis[k]) for k in range(3)) >= 0)
    else:
        big = max(range(3), key=lambda k: (abs(nrm[k]), -k))
        flip = nrm[big] < 0
    nrm = [-v if flip else v for v in nrm]
    conditioned = bool(eig[1] - eig[0] > mp.mpf(pc.GAP_FRACTION) * eig[2])
    d = -mp.fsum(nrm[k] * cen[k] for k in range(3))
    return dict(normal=[float(v) for v in nrm], d=float(d), centroid=[float(v) for v in cen], eig=[float(v) for v in eig], rmse=float(mp.sqrt(max(eig[0], 0))),
                conditioned=conditioned)


def evaluate_case(name, c, ties):
    cloud = c["cloud"]
    m, st = len(cloud), status_of(c)
    label = np.full(m, pc.NONE, dtype=np.uint32)
    alive = np.ones(m, dtype=bool) if not st else np.zeros(m, dtype=bool)
    planes = []
    if st == 0 and m:
        P, S = scaled_ints(cloud)
        for r in range(c["max_planes"]):
            rem = np.flatnonzero(alive)
            if len(rem) < max(3, c["min_inliers"]):
                break
            idx = np.array([pc.sample(c["seed"], r, h, len(rem)) for h in range(c["n_hyp"])], dtype=np.int64)
            assert (idx < len(rem)).all() and all(len(set(t)) == 3 for t in idx.tolist()), name
            inside = exact_round(name, P[rem], S, idx, c, ties)
            score = inside.sum(axis=1)
            w = int(np.argmax(score))                                           # the first among equals: the smallest h
            if score[w] < c["min_inliers"]:
                break
            if (score == score[w]).sum() > 1:
                ties["score"].add(name)
            members = rem[inside[w]]
            label[members] = r
            alive[members] = False
            fit = refit(cloud[members].astype(np.float64), c["axis"])
            fit.update(n_inliers=int(score[w]), hyp=w)
            planes.append(fit)
    on = int((label != pc.NONE).sum())
    keep = ((label != pc.NONE) if c["flags"] & pc.KEEP_PLANES else alive).astype(np.uint8)
    k = len(planes)
    u32 = lambda v: np.array([v], dtype=np.uint32)              # noqa: E731
    u64 = lambda v: np.array([v], dtype=np.uint64)              # noqa: E731
    col = lambda f, w: np.array([p[f] for p in planes], dtype=np.float64).reshape((k, w) if w > 1 else (k,))   # noqa: E731
    out = dict(label=label, keep=keep, n_inliers=np.array([p["n_inliers"] for p in planes], dtype=np.uint32), hyp=np.array([p["hyp"] for p in planes], dtype=np.uint32),
               conditioned=np.array([p["conditioned"] for p in planes], dtype=np.uint8), normal=col("normal", 3), d=col("d", 1), centroid=col("centroid", 3), eig=col("eig", 3),
               rmse=col("rmse", 1), n_on_planes=u64(on), n_rest=u64(0 if st else m - on), n_kept=u64(int(keep.sum())), n_planes=u32(k), status=u32(st))
    return {f"{name}/out/{k_}": v for k_, v in out.items()}


def evaluate(cases):
    out, ties = {}, dict(threshold=set(), score=set(), axis=set())
    for name, c in cases.items():
        out.update(evaluate_case(name, c, ties))
    order = list(cases)
    assert sorted(ties["threshold"], key=order.index) == sorted(pc.THRESHOLD_TIES, key=order.index), ("the cases with s*s == t2q", sorted(ties["threshold"], key=order.index))
    assert sorted(ties["score"], key=order.index) == sorted(pc.SCORE_TIES, key=order.index), ("the cases with several best hypotheses", sorted(ties["score"], key=order.index))
    assert sorted(ties["axis"]) == sorted(pc.AXIS_TIES), ("the cases with an exact tie of the axis test", sorted(ties["axis"]))
    return out


def inputs(cases):
    out = {"names": np.array(list(cases))}
    for name, c in cases.items():
        out[f"{name}/in/cloud"], out[f"{name}/in/dist"], out[f"{name}/in/cos_max_angle"] = c["cloud"], np.array([c["dist"]]), np.array([c["cos_max_angle"]])
        out[f"{name}/in/axis"] = np.array(c["axis"] if c["axis"] is not None else [], dtype=np.float64)
        out[f"{name}/in/seed"] = np.array([c["seed"]], dtype=np.uint64)
        for k in ("n_hyp", "max_planes", "min_inliers", "flags"):
            out[f"{name}/in/{k}"] = np.array([c[k]], dtype=np.uint32)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "planecloud_cases.npz")
    cases = pc.build()
    out = inputs(cases)
    out.update(evaluate(cases))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
