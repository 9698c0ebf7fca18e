"""Writes tests/golden/mme_cases.npz: the inputs of tests/mmecases.py::build() as float32 and, per case, what lk_clouds_mme_dev has to give.

    python tests/golden/make_mme_cases.py [path]

Decisions are taken in EXACT integer arithmetic: a float32 coordinate is an integer multiple of 2^-k, so with every coordinate of a cloud scaled by
one power of two S the offsets u about a point, d2 = u.u, the sums s and M over the members and  A = n M - s s^T  are Python integers, and
C = A / (n (n - 1) S^2), det C and tr C are exact rationals.  ln det, the smallest eigenvalue (trigonometric solution of the cubic) and the means
are then evaluated with mpmath at 50 digits and rounded to float64.  evaluate() ASSERTS what lets the tests compare every decision exactly - see
tests/mmecases.py for the list."""
import os
import sys
from fractions import Fraction

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mmecases as mc  # noqa: E402

mp.dps = 50
MARGIN = Fraction(1, 2 ** 40)
FLOOR = Fraction(1, 2 ** 30)
LN_2PIE_3 = 3 * (1 + mp.log(2 * mp.pi))


def status_of(c):
    v = c["cloud"].astype(np.float64)
    fin = np.isfinite(v)
    return (0 if fin.all() else 1) | (2 if (np.abs(v[fin] / c["radius"]) >= 2.0 ** 30).any() else 0)


def scaled_ints(cloud):
    """(P, S): the cloud as an object array of Python integers, P = cloud * S exactly, S a power of two."""
    den = 1
    for v in cloud.reshape(-1):
        den = max(den, float(v).as_integer_ratio()[1])
    return np.array([[int(Fraction(float(v)) * den) for v in row] for row in cloud], dtype=object).reshape(-1, 3), den


def smallest_eigenvalue(a):
    """of the symmetric integer matrix (a00 a01 a02 a11 a12 a22), positive semi-definite, at 50 digits"""
    a00, a01, a02, a11, a12, a22 = (mpf(v) for v in a)
    off = a01 * a01 + a02 * a02 + a12 * a12
    if off == 0:
        return min(a00, a11, a22)
    q = (a00 + a11 + a22) / 3
    b00, b11, b22 = a00 - q, a11 - q, a22 - q
    p = mp.sqrt((b00 * b00 + b11 * b11 + b22 * b22 + 2 * off) / 6)
    det = b00 * (b11 * b22 - a12 * a12) - a01 * (a01 * b22 - a12 * a02) + a02 * (a01 * a12 - b11 * a02)
    hd = max(mpf(-1), min(mpf(1), det / (2 * p * p * p)))
    return q + 2 * p * mp.cos(mp.acos(hd) / 3 + 2 * mp.pi / 3)


def evaluate_case(name, c):
    cloud, r, min_pts = c["cloud"], c["radius"], c["min_pts"]
    m, st = len(cloud), status_of(c)
    n = np.zeros(m, dtype=np.uint32)
    cls = np.zeros(m, dtype=np.uint8)
    h, lmin, kappa = np.full(m, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    h50, l50, tol50 = {}, {}, {}
    if st == 0 and m:
        P, S = scaled_ints(cloud)
        r2 = Fraction(r) * Fraction(r) * S * S                 # the exact square; the rounded product differs by 2^-53, inside MARGIN
        r2n, r2d = r2.numerator, r2.denominator
        for i in range(m):
            u = P - P[i]
            d2 = (u * u).sum(axis=1)
            lhs = d2 * r2d                                      # d2 <= r2  <=>  d2 * r2d <= r2n
            inside = (lhs <= r2n).astype(bool)
            near = np.flatnonzero([v != r2n and abs(v - r2n) * MARGIN.denominator < r2n for v in lhs])
            assert len(near) == 0, (name, i, "membership neither clear nor an exact tie", near)
            if any(v == r2n for v in lhs):
                assert float(r) * float(r) == Fraction(r) * Fraction(r), (name, i, "an exact tie under an inexact r * r")
            um = u[inside]
            k = int(len(um))
            n[i] = k
            if k < min_pts:
                continue
            s = um.sum(axis=0)
            pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
            A = [k * int((um[:, a] * um[:, b]).sum()) - int(s[a]) * int(s[b]) for a, b in pairs]
            a00, a01, a02, a11, a12, a22 = A
            detA = a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02) + a02 * (a01 * a12 - a11 * a02)
            trA = a00 + a11 + a22
            den = k * (k - 1) * S * S                           # C = A / den
            assert detA >= 0 and trA >= 0, (name, i)
            # flat: det C <= FLOOR (tr C / 3)^3  <=>  27 detA <= FLOOR trA^3
            flat = 27 * detA * FLOOR.denominator <= trA ** 3
            if trA:
                ratio = Fraction(27 * detA, trA ** 3)
                assert ratio <= FLOOR / 4 or ratio >= FLOOR * 4, (name, i, "flatness too close to the floor", float(ratio))
            l50[i] = (mpf(0) if detA == 0 else max(mpf(0), smallest_eigenvalue(A))) / den
            lmin[i] = float(l50[i])
            cls[i] = mc.FLAT if flat else mc.SCORED
            if not flat:
                h50[i] = (LN_2PIE_3 + mp.log(mpf(detA)) - 3 * mp.log(mpf(den))) / 2
                h[i] = float(h50[i])
                kappa[i] = float(mpf(trA) ** 3 / (27 * mpf(detA)))
                tol50[i] = mc.C_H * mc.ULP * (kappa[i] + abs(h[i]))
    dense, scored = np.flatnonzero(cls != mc.SPARSE), np.flatnonzero(cls == mc.SCORED)
    mme = mpv = h_max = float("nan")
    worst = 0
    if len(dense):
        mpv = float(sum(l50[i] for i in dense) / len(dense))
    if len(scored):
        mme = float(sum(h50[i] for i in scored) / len(scored))
        order = sorted(scored, key=lambda i: (-h50[i], i))
        worst, h_max = int(order[0]), float(h50[order[0]])
        if len(order) > 1:
            a, b = order[0], order[1]
            if not np.array_equal(cloud[a], cloud[b]):          # duplicates of one point walk the same records: equal bits
                assert h50[a] - h50[b] >= 4 * max(tol50[a], tol50[b]), (name, "worst: neither clear nor a duplicate", a, b, float(h50[a] - h50[b]))
    out = dict(n=n, cls=cls, h=h, lmin=lmin, kappa=kappa, mme=np.array([mme]), mpv=np.array([mpv]), h_max=np.array([h_max]),
               n_dense=np.array([len(dense)], dtype=np.uint64), n_scored=np.array([len(scored)], dtype=np.uint64),
               n_pairs=np.array([int(n.astype(np.uint64).sum())], dtype=np.uint64), worst=np.array([worst], dtype=np.uint32),
               status=np.array([st], dtype=np.uint32))
    return {f"{name}/out/{k}": v for k, v in out.items()}


def evaluate(cases):
    out = {}
    for name, c in cases.items():
        out.update(evaluate_case(name, c))
    return out


def inputs(cases):
    out = {"names": np.array(list(cases))}
    for name, c in cases.items():
        out[f"{name}/in/cloud"] = c["cloud"]
        out[f"{name}/in/radius"], out[f"{name}/in/min_pts"] = np.array([c["radius"]]), np.array([c["min_pts"]], dtype=np.uint32)
    return out


def ratios(cases, gold, fn):
    """Worst error / (bound at C = 1) of fn(cloud, radius, min_pts) over the table - ((ratio_h, where), (ratio_l, where)); its decisions are asserted.
    fn returns cloudmetrics.mme's dict."""
    worst_h, worst_l = (0.0, None), (0.0, None)
    for name, c in cases.items():
        g, got = gold[name], fn(c["cloud"], c["radius"], c["min_pts"])
        assert np.array_equal(got["n"], g["n"]) and np.array_equal(got["cls"], g["cls"]), name
        for k in mc.COUNTS:
            assert int(got[k]) == g[k], (name, k, got[k], g[k])
        assert np.array_equal(np.isnan(got["h"]), np.isnan(g["h"])) and np.array_equal(np.isnan(got["lmin"]), np.isnan(g["lmin"])), name
        th, tl = mc.tol_h(g, 1.0), mc.tol_lmin(c, 1.0)
        rec_tol = mc.tol_record(c, g, 1.0, 1.0)
        cand_h = [(abs(got["h"][i] - g["h"][i]) / th[i], (name, "h", int(i))) for i in np.flatnonzero(g["cls"] == mc.SCORED)]
        cand_l = [(abs(got["lmin"][i] - g["lmin"][i]) / tl, (name, "lmin", int(i))) for i in np.flatnonzero(g["cls"] != mc.SPARSE)]
        for f, t, cand in (("mme", rec_tol[0], cand_h), ("mpv", rec_tol[1], cand_l), ("h_max", rec_tol[2], cand_h)):
            assert np.isnan(got[f]) == np.isnan(g[f]), (name, f)
            if not np.isnan(g[f]):
                cand.append((abs(got[f] - g[f]) / t, (name, f)))
        worst_h, worst_l = max([worst_h] + cand_h, key=lambda v: v[0]), max([worst_l] + cand_l, key=lambda v: v[0])
    return worst_h, worst_l


def golden_of(ev, cases):
    out = {}
    for n in cases:
        g = {k: ev[f"{n}/out/{k}"] for k in mc.PER_POINT}
        g.update({k: float(ev[f"{n}/out/{k}"][0]) for k in mc.FIGURES})
        g.update({k: int(ev[f"{n}/out/{k}"][0]) for k in mc.COUNTS})
        out[n] = g
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lk_pkg  # noqa: E402

    lk_pkg.load()
    from legkilo_amd import cloudmetrics

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mme_cases.npz")
    cases = mc.build()
    out = inputs(cases)
    ev = evaluate(cases)
    (rh, wh), (rl, wl) = ratios(cases, golden_of(ev, cases), cloudmetrics.mme)
    print(f"numpy restatement: NUMPY_RATIO_H {rh:.3f} at {wh}, NUMPY_RATIO_L {rl:.3f} at {wl}")
    out.update(ev)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
