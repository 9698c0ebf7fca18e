"""Writes tests/golden/sor_cases.npz: the inputs of tests/sorcases.py::build() as float32 and, per case, what lk_clouds_sor_dev has to give.

    python tests/golden/make_sor_cases.py [path]

Decisions are taken in EXACT integer arithmetic: a float32 coordinate is an integer multiple of 2^-k, so with every coordinate of a cloud scaled by
one power of two S every d2 is a Python integer; membership, cnt_i and the k smallest d2 of a point are found without rounding.  Their roots, dbar_i,
mu, sigma and thr are then evaluated with mpmath at 50 digits and rounded to float64.  evaluate() ASSERTS what lets the tests compare every decision
exactly - see tests/sorcases.py for the list."""
import os
import sys
from fractions import Fraction

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sorcases as sc  # noqa: E402

mp.dps = 50
MARGIN = 2 ** 40


def status_of(c):
    v = c["cloud"].astype(np.float64)
    fin = np.isfinite(v)
    return (0 if fin.all() else 1) | (2 if (np.abs(v[fin] / c["reach"]) >= 2.0 ** 30).any() else 0)


def scaled_ints(cloud):
    """(P, S): the cloud as an object array of Python integers, P = cloud * S exactly, S a power of two."""
    den = 1
    for v in cloud.reshape(-1):
        den = max(den, float(v).as_integer_ratio()[1])
    return np.array([[int(Fraction(float(v)) * den) for v in row] for row in cloud], dtype=object).reshape(-1, 3), den


def evaluate_case(name, c):
    cloud, k, r, n_sigma = c["cloud"], c["k"], c["reach"], c["n_sigma"]
    m, st = len(cloud), status_of(c)
    cnt = np.zeros(m, dtype=np.uint32)
    keep = np.zeros(m, dtype=np.uint8)
    dbar = np.full(m, np.nan)
    d50, least = {}, {}
    if st == 0 and m:
        P, S = scaled_ints(cloud)
        r2 = Fraction(r) * Fraction(r) * S * S                 # the exact square; the rounded product differs by 2^-53, inside the margin
        r2n, r2d = r2.numerator, r2.denominator
        for i in range(m):
            u = P - P[i]
            d2 = (u * u).sum(axis=1)
            lhs = d2 * r2d                                      # d2 <= r2  <=>  d2 * r2d <= r2n
            assert not any(v != r2n and abs(v - r2n) * MARGIN < r2n for v in lhs), (name, i, "membership neither clear nor an exact tie")
            if any(v == r2n for v in lhs):
                assert float(r) * float(r) == Fraction(r) * Fraction(r), (name, i, "an exact tie under an inexact reach * reach")
            cand = sorted(int(d2[j]) for j in range(m) if j != i and lhs[j] <= r2n)   # exclusion by index
            cnt[i] = len(cand)
            if len(cand) < k:
                continue
            least[i] = tuple(cand[:k])
            d50[i] = sum(mp.sqrt(mpf(v)) for v in least[i]) / (k * S)
            dbar[i] = float(d50[i])
    ok = sorted(d50)
    mu = sigma = thr = float("nan")
    worst = 0
    if ok:
        n_s = len(ok)
        mu50 = sum(d50[i] for i in ok) / n_s
        sigma50 = mp.sqrt(sum((d50[i] - mu50) ** 2 for i in ok) / (n_s - 1)) if n_s > 1 else mpf(0)
        thr50 = mp.inf if n_sigma == float("inf") else mu50 + mpf(n_sigma) * sigma50
        mu, sigma, thr = float(mu50), float(sigma50), float(thr50)
        g = dict(sigma=sigma)
        tol = sc.tol_d(c) + (sc.tol_s(c, g) if sigma > 0.0 else sc.tol_d(c))
        same = all(least[i] == least[ok[0]] for i in ok)        # every dbar the same exact number: dbar = mu = thr, sigma = 0
        for i in ok:
            keep[i] = 1 if d50[i] <= thr50 else 0
            if thr50 != mp.inf and not same:
                assert abs(d50[i] - thr50) >= 1024 * tol, (name, i, "dbar too close to thr", float(d50[i]), thr)
        order = sorted(ok, key=lambda i: (-d50[i], i))
        worst = int(order[0])
        if len(order) > 1 and least[order[0]] != least[order[1]]:
            assert d50[order[0]] - d50[order[1]] >= 4 * sc.tol_d(c), (name, "worst not clear", order[:2])
    n_kept = int(keep.sum())
    out = dict(cnt=cnt, keep=keep, dbar=dbar, mu=np.array([mu]), sigma=np.array([sigma]), thr=np.array([thr]),
               n_isolated=np.array([0 if st else m - len(ok)], dtype=np.uint64), n_outliers=np.array([len(ok) - n_kept], dtype=np.uint64),
               n_kept=np.array([n_kept], dtype=np.uint64), worst=np.array([worst], dtype=np.uint32), status=np.array([st], dtype=np.uint32))
    return {f"{name}/out/{k_}": v for k_, v in out.items()}


def evaluate(cases):
    out = {}
    for name, c in cases.items():
        out.update(evaluate_case(name, c))
    return out


def inputs(cases):
    out = {"names": np.array(list(cases))}
    for name, c in cases.items():
        out[f"{name}/in/cloud"] = c["cloud"]
        out[f"{name}/in/k"], out[f"{name}/in/reach"] = np.array([c["k"]], dtype=np.uint32), np.array([c["reach"]])
        out[f"{name}/in/n_sigma"] = np.array([c["n_sigma"]])
    return out


def ratios(cases, gold, fn):
    """Worst error / (bound at C = 1) of fn(cloud, k, reach, n_sigma) over the table - ((ratio_d, where), (ratio_s, where)); its decisions are
    asserted.  fn returns cloudmetrics.sor's dict."""
    worst_d, worst_s = (0.0, None), (0.0, None)
    for name, c in cases.items():
        g, got = gold[name], fn(c["cloud"], c["k"], c["reach"], c["n_sigma"])
        assert np.array_equal(got["cnt"], g["cnt"]) and np.array_equal(np.asarray(got["keep"], dtype=np.uint8), g["keep"]), name
        for k_ in sc.COUNTS:
            assert int(got[k_]) == g[k_], (name, k_, got[k_], g[k_])
        assert np.array_equal(np.isnan(got["dbar"]), np.isnan(g["dbar"])), name
        td, ts = sc.tol_d(c, 1.0), sc.tol_s(c, g, 1.0)
        has = ~np.isnan(g["dbar"])
        cand_d = [(abs(got["dbar"][i] - g["dbar"][i]) / td, (name, "dbar", int(i))) for i in np.flatnonzero(has)]
        cand_s = []
        for f in sc.FIGURES:
            assert np.isnan(got[f]) == np.isnan(g[f]), (name, f)
        if has.any():
            cand_d.append((abs(got["mu"] - g["mu"]) / td, (name, "mu")))
            if g["sigma"] > 0.0:
                cand_s.append((abs(got["sigma"] - g["sigma"]) / ts, (name, "sigma")))
            else:
                assert got["sigma"] == 0.0, (name, "sigma")
            if np.isinf(g["thr"]):
                assert got["thr"] == g["thr"], (name, "thr")
            elif g["sigma"] > 0.0:
                cand_s.append((abs(got["thr"] - g["thr"]) / ts, (name, "thr")))
            else:
                cand_d.append((abs(got["thr"] - g["thr"]) / td, (name, "thr")))
        worst_d, worst_s = max([worst_d] + cand_d, key=lambda v: v[0]), max([worst_s] + cand_s, key=lambda v: v[0])
    return worst_d, worst_s


def golden_of(ev, cases):
    out = {}
    for n in cases:
        g = {k: ev[f"{n}/out/{k}"] for k in sc.PER_POINT}
        g.update({k: float(ev[f"{n}/out/{k}"][0]) for k in sc.FIGURES})
        g.update({k: int(ev[f"{n}/out/{k}"][0]) for k in sc.COUNTS})
        out[n] = g
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lk_pkg  # noqa: E402

    lk_pkg.load()
    from legkilo_amd import cloudmetrics

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sor_cases.npz")
    cases = sc.build()
    out = inputs(cases)
    ev = evaluate(cases)
    (rd, wd), (rs, ws) = ratios(cases, golden_of(ev, cases), cloudmetrics.sor)
    print(f"numpy restatement: NUMPY_RATIO_D {rd:.3f} at {wd}, NUMPY_RATIO_S {rs:.3f} at {ws}")
    out.update(ev)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
