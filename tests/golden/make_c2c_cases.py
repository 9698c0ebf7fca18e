"""Writes tests/golden/c2c_cases.npz: the inputs of tests/c2ccases.py::build() as float32 and, per case, what lk_clouds_c2c_dev has to give -
decided and evaluated with mpmath at 50 digits from the float coordinates (a coordinate difference, its square and the sum of three are exact there).

    python tests/golden/make_c2c_cases.py [path]

evaluate() ASSERTS what lets the tests compare every decision exactly (MARGIN = 2^-40, relative):
  * nearest neighbour of every matched point: the runner-up's d2 is either MARGIN above the best, or exactly equal to it with equal rounded float64
    values (then the smallest index is the answer);
  * matched, and every threshold: d2 is MARGIN away from max_dist^2 (thr^2), or exactly equal with the rounded values equal;
  * worst: the largest matched d2 leads the runner-up by MARGIN, or ties exactly as above (then the first index).
A float64 pre-filter picks the candidates that go to 50 digits: a reference point whose rounded d2 lies 2^-30 above the rounded minimum cannot be the
best or a runner-up inside MARGIN (the rounded value is within 2^-50 of the exact one)."""
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import c2ccases as cc  # noqa: E402

mp.dps = 50
MARGIN = mpf(2) ** -40


def exact_d2(q, r):
    dx, dy, dz = (mpf(float(a)) - mpf(float(b)) for a, b in zip(q, r))
    return dx * dx + dy * dy + dz * dz


def rounded_d2(q, r):
    d = q.astype(np.float64) - r.astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def clear_or_tie(lo, hi, lo_rounded, hi_rounded, what):
    """lo <= hi at 50 digits: apart by MARGIN, or exactly equal with equal rounded values.  Returns True for a tie."""
    if lo == hi:
        assert lo_rounded == hi_rounded, (what, "an exact tie whose rounded values differ")
        return True
    assert hi - lo >= MARGIN * hi, (what, "neither clear nor an exact tie", float(lo), float(hi))
    return False


def status_of(c):
    st = 0
    for a in (c["query"], c["ref"]):
        v = a.astype(np.float64)
        fin = np.isfinite(v)
        st |= 0 if fin.all() else 1
        st |= 2 if (np.abs(v[fin] / c["max_dist"]) >= 2.0 ** 30).any() else 0
    return st


def evaluate_case(name, c):
    q, r, md = c["query"], c["ref"], c["max_dist"]
    n, st = len(q), status_of(c)
    j = np.full(n, cc.NO_MATCH, dtype=np.uint32)
    matched = np.zeros(n, dtype=bool)
    reach2, reach2_rounded = mpf(md) * mpf(md), md * md
    best = [None] * n
    if st == 0 and len(r):
        for i in range(n):
            rd = rounded_d2(q[i], r)
            cand = np.flatnonzero(rd <= rd.min() * (1.0 + 2.0 ** -30))
            ex = sorted((exact_d2(q[i], r[k]), int(k)) for k in cand)
            e0, k0 = ex[0]
            if e0 != reach2:
                inside = e0 < reach2
                clear_or_tie(min(e0, reach2), max(e0, reach2), 0, 0, (name, i, "matched"))
            else:
                inside = clear_or_tie(e0, reach2, rd[k0], reach2_rounded, (name, i, "matched"))
            if not inside:
                continue
            if len(ex) > 1:
                clear_or_tie(e0, ex[1][0], rd[k0], rd[ex[1][1]], (name, i, "runner-up"))
            matched[i], j[i], best[i] = True, k0, (e0, float(rd[k0]))
    mi = np.flatnonzero(matched)
    within = []
    for t in c["thr"]:
        t2, t2r, cnt = mpf(float(t)) * mpf(float(t)), float(t) * float(t), 0
        for i in mi:
            e, er = best[i]
            if e == t2:
                cnt += clear_or_tie(e, t2, er, t2r, (name, int(i), "threshold"))
            else:
                clear_or_tie(min(e, t2), max(e, t2), 0, 0, (name, int(i), "threshold"))
                cnt += e < t2
        within.append(cnt)
    rmse = mean = mx = float("nan")
    worst = 0
    if len(mi):
        es = [best[i][0] for i in mi]
        rmse, mean, mx = float(mp.sqrt(sum(es) / len(es))), float(sum(mp.sqrt(e) for e in es) / len(es)), float(mp.sqrt(max(es)))
        order = sorted(range(len(es)), key=lambda k: (-es[k], k))
        worst = int(mi[order[0]])
        if len(es) > 1:
            a, b = order[0], order[1]
            clear_or_tie(es[b], es[a], best[mi[b]][1], best[mi[a]][1], (name, "worst"))
    out = dict(j=j, matched=matched, n_within=np.array(within, dtype=np.uint64), rmse=np.array([rmse]), mean=np.array([mean]), max=np.array([mx]),
               n_matched=np.array([len(mi)], dtype=np.uint64), worst=np.array([worst], dtype=np.uint32), status=np.array([st], dtype=np.uint32))
    return {f"{name}/out/{k}": v for k, v in out.items()}


def evaluate(cases):
    out = {}
    for name, c in cases.items():
        out.update(evaluate_case(name, c))
    return out


def inputs(cases):
    out = {"names": np.array(list(cases))}
    for name, c in cases.items():
        out[f"{name}/in/query"], out[f"{name}/in/ref"] = c["query"], c["ref"]
        out[f"{name}/in/max_dist"], out[f"{name}/in/thr"] = np.array([c["max_dist"]]), c["thr"]
    return out


def numpy_ratio(cases, ev):
    """Worst |x_numpy - x_50| / (2^-53 max_dist) of legkilo_amd.cloudmetrics.c2c over the table's figures, with where; its decisions are asserted."""
    from legkilo_amd import cloudmetrics

    worst = (0.0, None)
    for name, c in cases.items():
        got = cloudmetrics.c2c(c["query"], c["ref"], c["max_dist"], c["thr"])
        assert np.array_equal(got["j"], ev[f"{name}/out/j"]) and np.array_equal(got["matched"], ev[f"{name}/out/matched"]), name
        assert list(got["n_within"]) == list(ev[f"{name}/out/n_within"]) and got["worst"] == ev[f"{name}/out/worst"][0], name
        assert got["status"] == ev[f"{name}/out/status"][0] and got["n_matched"] == ev[f"{name}/out/n_matched"][0], name
        for f in ("rmse", "mean", "max"):
            want = ev[f"{name}/out/{f}"][0]
            assert np.isnan(want) == np.isnan(got[f]), (name, f)
            if not np.isnan(want):
                ratio = abs(got[f] - want) / (cc.ULP * c["max_dist"])
                if ratio > worst[0]:
                    worst = (ratio, (name, f))
    return worst


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lk_pkg  # noqa: E402

    lk_pkg.load()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "c2c_cases.npz")
    cases = cc.build()
    out = inputs(cases)
    ev = evaluate(cases)
    ratio, where = numpy_ratio(cases, ev)
    print(f"numpy restatement: NUMPY_RATIO {ratio:.3f} at {where}")
    out.update(ev)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
