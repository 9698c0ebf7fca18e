"""Writes tests/golden/align_cases.npz: the inputs of tests/aligncases.py::build() and, per case, what lk_clouds_align_dev has to give - its
definition (include/legkilo_hip.h) run with mpmath at 50 digits from the float coordinates and the float64 T0.

    python tests/golden/make_align_cases.py [path]

evaluate_case() ASSERTS what lets the tests compare every decision exactly.  With the tolerance granted to T (aligncases.C_R, C_T; L the pair's
largest coordinate) a moved point may be off by dm = (3 C_R + C_T) 2^-53 L, a distance by as much.  MARGIN = 2^10:
  * nearest neighbour, every search of every iteration: the runner-up's distance is MARGIN dm above the best, or its d2 is exactly equal with the
    float64 values (under the rounded T) equal as well - then the smallest index is the answer;
  * matched, every search: the best distance is MARGIN dm away from max_dist; the range guard: |m / max_dist| is 1 away from 2^30;
  * n >= 3: an integer, clear once the matched flags are;
  * the stop comparisons, every solve: step_rot is MARGIN 4 C_R 2^-53 away from eps_rot and step_trans MARGIN 2 dm from eps_trans, or the step is
    exactly 0 - a solve that repeats the one before it, which in float64 repeats to the bit as well (lk_align.h);
  * thresholds and worst of the final search as in make_c2c_cases.py, with MARGIN dm on distances.
For the posed cases it asserts that in every solve Horn's largest eigenvalue is separated from the next by a tenth of the spread (`gap`); a free
case (a line) where it is not gets clear = 0, and the tests then compare nothing that the free direction decides.
c2c_tie = 1: no final distance lies within 4 * 2^-24 * L of max_dist and no runner-up within that of the best, so lk_clouds_c2c_dev on the
float32 rounding of the moved cloud takes the same decisions (each coordinate moves by at most half a float32 ulp of L)."""
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import aligncases as ac  # noqa: E402

mp.dps = 50
MARGIN = 2.0 ** 10


def f64_d2(m, r):
    d = m - r.astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def f64_move(T, p):
    p = p.astype(np.float64)
    return np.stack([((T[3 * a] * p[:, 0] + T[3 * a + 1] * p[:, 1]) + T[3 * a + 2] * p[:, 2]) + T[9 + a] for a in range(3)], axis=1)


def status_of(c):
    st = 0
    for a in (c["query"], c["ref"]):
        v = a.astype(np.float64)
        fin = np.isfinite(v)
        st |= 0 if fin.all() else 1
        st |= 2 if (np.abs(v[fin] / c["max_dist"]) >= 2.0 ** 30).any() else 0
    return st | (0 if np.isfinite(c["T0"]).all() else ac.BAD_T0)


def search(name, c, T, dm, what):
    """One search under T (12 mpf) -> (j uint32 [n], matched bool [n], exact d2 per point or None, tie_ok)."""
    q, r, md = c["query"], c["ref"], c["max_dist"]
    n = len(q)
    j, matched, best = np.full(n, ac.NO_MATCH, dtype=np.uint32), np.zeros(n, dtype=bool), [None] * n
    Tf = np.array([float(v) for v in T])
    mf = f64_move(Tf, q)
    reach2, reach2_f = mpf(md) * mpf(md), md * md
    pad32 = 4.0 * 2.0 ** -24 * ac.extent(c)
    tie_ok = True
    for i in range(n):
        p = [mpf(float(v)) for v in q[i]]
        m = [T[3 * a] * p[0] + T[3 * a + 1] * p[1] + T[3 * a + 2] * p[2] + T[9 + a] for a in range(3)]
        cells = [abs(v / mpf(md)) for v in m]
        assert all(abs(v - mpf(2) ** 30) > 1 for v in cells), (name, what, i, "the range guard is not clear")
        if any(v >= mpf(2) ** 30 for v in cells) or not len(r):
            continue
        dist = np.sqrt(f64_d2(mf[i], r))
        cand = np.flatnonzero(dist <= dist.min() + max(4.0 * MARGIN * dm, 2.0 * pad32, 1e-9))
        ex = sorted((sum((m[a] - mpf(float(r[k][a]))) ** 2 for a in range(3)), int(k)) for k in cand)
        e0, k0 = ex[0]
        d0 = mp.sqrt(e0)
        if e0 == reach2:
            assert f64_d2(mf[i], r[k0]) == reach2_f, (name, what, i, "matched: an exact tie whose rounded values differ")
            inside = True
        else:
            assert abs(d0 - md) >= MARGIN * dm, (name, what, i, "matched: neither clear nor an exact tie", float(d0))
            inside = e0 < reach2
        tie_ok = tie_ok and abs(d0 - md) > pad32
        if not inside:
            continue
        if len(ex) > 1:
            e1, k1 = ex[1]
            if e1 == e0:
                assert f64_d2(mf[i], r[k0]) == f64_d2(mf[i], r[k1]), (name, what, i, "runner-up: an exact tie whose rounded values differ")
            else:
                assert mp.sqrt(e1) - d0 >= MARGIN * dm, (name, what, i, "runner-up: neither clear nor an exact tie", float(d0), float(mp.sqrt(e1)))
            tie_ok = tie_ok and (e1 == e0 or mp.sqrt(e1) - d0 > pad32)
        j[i], matched[i], best[i] = k0, True, e0
    return j, matched, best, tie_ok


def horn(S):
    """(R as 9 mpf, gap) of the 3 x 3 mpf matrix S: the eigenvector of the largest eigenvalue of Horn's N; gap = (l1 - l2) / (l1 - l4)."""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = mp.matrix([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                   [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy], [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    E, Q = mp.eigsy(N)
    order = sorted(range(4), key=lambda k: E[k])
    top = order[3]
    w, x, y, z = (Q[k, top] for k in range(4))
    nrm = mp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    spread = E[order[3]] - E[order[0]]
    gap = float((E[order[3]] - E[order[2]]) / spread) if spread > 0 else 0.0
    R = [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), w * w + y * y - x * x - z * z, 2 * (y * z - w * x),
         2 * (x * z - w * y), 2 * (y * z + w * x), w * w + z * z - x * x - y * y]
    return R, gap


def figures(name, c, matched, best, dm):
    """rmse, mean, max, n_within, worst of one search's exact d2, the threshold and worst decisions asserted clear."""
    mi = np.flatnonzero(matched)
    if not len(mi):
        return float("nan"), float("nan"), float("nan"), [0] * len(c["thr"]), 0
    es = [best[i] for i in mi]
    ds = [mp.sqrt(e) for e in es]
    within = []
    for t in c["thr"]:
        t = float(t)
        for d in ds:
            assert abs(d - t) >= MARGIN * dm or (t == c["max_dist"] and d <= t), (name, "threshold", t, float(d))
        within.append(int(sum(d <= t for d in ds)))
    order = sorted(range(len(es)), key=lambda k: (-es[k], k))
    if len(es) > 1 and es[order[0]] != es[order[1]]:
        assert ds[order[0]] - ds[order[1]] >= MARGIN * dm, (name, "worst", float(ds[order[0]]), float(ds[order[1]]))
    return float(mp.sqrt(sum(es) / len(es))), float(sum(ds) / len(ds)), float(ds[order[0]]), within, int(mi[order[0]])


def evaluate_case(name, c):
    q, r, md = c["query"], c["ref"], c["max_dist"]
    n, L, st = len(q), ac.extent(c), status_of(c)
    dm = (3.0 * ac.C_R + ac.C_T) * ac.ULP * L
    nan = float("nan")
    out = dict(T=c["T0"].copy(), j_first=np.full(n, ac.NO_MATCH, dtype=np.uint32), matched_first=np.zeros(n, dtype=bool), j=np.full(n, ac.NO_MATCH, dtype=np.uint32),
               matched=np.zeros(n, dtype=bool), n_within=np.zeros(len(c["thr"]), dtype=np.uint64), rmse_first=nan, step_rot=nan, step_trans=nan, rmse=nan, mean=nan,
               max=nan, gap=nan, iters=0, status=st, n_matched_first=0, n_matched=0, worst=0, clear=1, c2c_tie=0)
    if not st:
        T = [mpf(float(v)) for v in c["T0"]]
        iters, stopped, first, gaps = 0, False, True, []
        while True:
            j, m, best, tie_ok = search(name, c, T, dm, f"search {iters}")
            if first:
                first = False
                out["j_first"], out["matched_first"], out["n_matched_first"] = j.copy(), m.copy(), int(m.sum())
                out["rmse_first"] = figures(name, c, m, best, dm)[0]
            if iters == c["max_iter"] or stopped:
                break
            if m.sum() < 3:
                st |= ac.FEW
                break
            mi = np.flatnonzero(m)
            P = [[mpf(float(v)) for v in q[i]] for i in mi]
            G = [[mpf(float(v)) for v in r[j[i]]] for i in mi]
            cnt = len(mi)
            pbar = [sum(p[a] for p in P) / cnt for a in range(3)]
            rbar = [sum(g[a] for g in G) / cnt for a in range(3)]
            S = [[sum((p[a] - pbar[a]) * (g[b] - rbar[b]) for p, g in zip(P, G)) for b in range(3)] for a in range(3)]
            Rn, gap = horn(S)
            gaps.append(gap)
            Tn = Rn + [rbar[a] - (Rn[3 * a] * pbar[0] + Rn[3 * a + 1] * pbar[1] + Rn[3 * a + 2] * pbar[2]) for a in range(3)]
            E = [[Tn[3 * i] * T[3 * k] + Tn[3 * i + 1] * T[3 * k + 1] + Tn[3 * i + 2] * T[3 * k + 2] for k in range(3)] for i in range(3)]
            v = [E[2][1] - E[1][2], E[0][2] - E[2][0], E[1][0] - E[0][1]]
            s, co = mpf(0.5) * mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), mpf(0.5) * (E[0][0] + E[1][1] + E[2][2] - 1)
            step_rot = mp.atan2(s, co)
            mv = lambda X: [X[3 * a] * pbar[0] + X[3 * a + 1] * pbar[1] + X[3 * a + 2] * pbar[2] + X[9 + a] for a in range(3)]   # noqa: E731
            step_trans = mp.sqrt(sum((x - y) ** 2 for x, y in zip(mv(Tn), mv(T))))
            if gap >= 0.1:
                same = all(x == y for x, y in zip(T, Tn))
                assert (same and step_rot == 0) or abs(step_rot - c["eps_rot"]) >= MARGIN * 4.0 * ac.C_R * ac.ULP, (name, iters, "step_rot is not clear", float(step_rot))
                assert (same and step_trans == 0) or abs(step_trans - c["eps_trans"]) >= MARGIN * 2.0 * dm, (name, iters, "step_trans is not clear", float(step_trans))
            T, iters = Tn, iters + 1
            out["step_rot"], out["step_trans"] = float(step_rot), float(step_trans)
            if step_rot <= c["eps_rot"] and step_trans <= c["eps_trans"]:
                st |= ac.CONVERGED
                stopped = True
        rmse, mean, mx, within, worst = figures(name, c, m, best, dm)
        out.update(T=np.array([float(v) for v in T]) if iters else c["T0"].copy(), j=j, matched=m, n_within=np.array(within, dtype=np.uint64), rmse=rmse, mean=mean, max=mx,
                   iters=iters, status=st, n_matched=int(m.sum()), worst=worst, gap=min(gaps) if gaps else nan, clear=int(all(g >= 0.1 for g in gaps)),
                   c2c_tie=int(tie_ok and iters > 0))
        if c["kind"] == "posed":
            assert out["clear"], (name, "a posed case whose Horn eigenvalues are not separated", gaps)
    dt = dict(T=np.float64, j_first=np.uint32, matched_first=bool, j=np.uint32, matched=bool, n_within=np.uint64)
    res = {}
    for k in ac.OUT_ARRAYS:
        res[f"{name}/out/{k}"] = np.asarray(out[k], dtype=dt[k])
    for k in ac.OUT_FLOATS:
        res[f"{name}/out/{k}"] = np.array([out[k]], dtype=np.float64)
    for k in ac.OUT_INTS:
        res[f"{name}/out/{k}"] = np.array([out[k]], dtype=np.int64)
    return res


def evaluate(cases):
    out = {}
    for name, c in cases.items():
        out.update(evaluate_case(name, c))
    return out


def inputs(cases):
    out = {"names": np.array(list(cases))}
    for name, c in cases.items():
        for k in ("query", "ref", "thr", "T0"):
            out[f"{name}/in/{k}"] = c[k]
        for k, dt in (("max_dist", np.float64), ("eps_rot", np.float64), ("eps_trans", np.float64), ("max_iter", np.int64), ("has_T0", bool)):
            out[f"{name}/in/{k}"] = np.array([c[k]], dtype=dt)
        out[f"{name}/in/kind"] = np.array([c["kind"]])
    return out


def golden_of(ev, name):
    g = {k: ev[f"{name}/out/{k}"] for k in ac.OUT_ARRAYS}
    g.update({k: float(ev[f"{name}/out/{k}"][0]) for k in ac.OUT_FLOATS})
    g.update({k: int(ev[f"{name}/out/{k}"][0]) for k in ac.OUT_INTS})
    return g


def run_numpy(c, variant=None):
    """legkilo_amd.cloudmetrics.align of one case in the shape aligncases.compare takes."""
    from legkilo_amd import cloudmetrics

    a = cloudmetrics.align(c["query"], c["ref"], c["max_dist"], c["T0"] if c["has_T0"] else None, c["max_iter"], c["eps_rot"], c["eps_trans"], c["thr"], variant=variant)
    f = a["c2c"]
    return dict(T=a["T"], iters=a["iters"], status=a["status"], n_matched_first=a["n_matched_first"], rmse_first=a["rmse_first"], step_rot=a["step_rot"],
                step_trans=a["step_trans"], rmse=f["rmse"], mean=f["mean"], max=f["max"], n_matched=f["n_matched"], n_within=f["n_within"], worst=f["worst"],
                j_first=a["first"][0], matched_first=a["first"][1], j=f["j"], matched=f["matched"])


def numpy_ratios(cases, ev):
    """Worst ratios of legkilo_amd.cloudmetrics.align over the table, with where: {"R": (ratio, case), "T": ..., "FIG": ...}; its decisions are asserted."""
    worst = {k: (0.0, None) for k in ("R", "T", "FIG")}
    for name, c in cases.items():
        got = ac.compare(name, run_numpy(c), golden_of(ev, name), c)
        for k, v in got.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    return worst


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lk_pkg  # noqa: E402

    lk_pkg.load()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "align_cases.npz")
    cases = ac.build()
    out = inputs(cases)
    ev = evaluate(cases)
    for name in cases:
        g = golden_of(ev, name)
        print(f"{name:12s} iters {g['iters']:2d} status {g['status']:2d} matched {g['n_matched_first']:3d} -> {g['n_matched']:3d} rmse {g['rmse_first']:.3e} -> {g['rmse']:.3e} "
              f"gap {g['gap']:.3f} clear {g['clear']} c2c_tie {g['c2c_tie']}")
    for k, (ratio, where) in numpy_ratios(cases, ev).items():
        print(f"numpy restatement: RATIO_{k} {ratio:.3f} at {where}")
    out.update(ev)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
