"""Writes tests/golden/rpe_cases.npz: the inputs of every case of tests/rpecases.py as build() gives them here (`name/in/...`), and each case
under each of its modes evaluated at 50 digits (mpmath) from exactly those float64 bits by the definition of lk_traj_rpe_dev in include/legkilo_hip.h,
rounded to float64 (`name/m<q>/...`): the six figures, n_terms / n_pairs / status / worst_trans / worst_rot, the term list (i, k, a, b) with e_t and
e_r per term, the margins by which the worst terms lead their runners-up, and the tolerance scales S and M - all packed by rpecases.pack into four
arrays.  Partner and step are decided on the float64 stamps with the one rounded subtraction / addition the definition states them in.

    python tests/golden/make_rpe_cases.py [out.npz]

Beside writing, the script asserts what tests/rpecases.py promises about the worst terms and measures the ratios the numpy restatement tum.rpe reaches
(NUMPY_RATIO_T, NUMPY_RATIO_R there).  The figures are a function of the frozen inputs alone: tests/test_rpe_host.py runs evaluate() on them again and
compares bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import rpecases as rc  # noqa: E402


def partners(c):
    out = np.full(len(c["est_t"]), -1, dtype=np.int64)
    gt = c["gt_t"]
    if len(gt):
        for i, te in enumerate(c["est_t"]):
            d = np.abs(te - gt)          # "one rounded subtraction": the rule is about this float64 value
            j = int(np.argmin(d))        # the first of equal minima
            if d[j] <= c["max_dt"]:
                out[i] = j
    return out


def steps(c, delta, flags):
    t = c["est_t"]
    n = len(t)
    out = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        if flags:
            k = i + int(delta)
        else:
            target = t[i] + delta        # "one rounded addition"
            k = next((k for k in range(i + 1, n) if t[k] >= target), n)
        if k < n:
            out[i] = k
    return out


def evaluate_mode(c, delta, flags, mp):
    part, step = partners(c), steps(c, delta, flags)
    terms = np.array([(i, k, part[i], part[k]) for i, k in enumerate(step) if k >= 0 and part[i] >= 0 and part[k] >= 0], dtype=np.int64).reshape(-1, 4)
    nan = float("nan")
    n = len(terms)
    res = dict(figures=np.full(6, nan), counts=np.array([n, int((part >= 0).sum()), 0, 0, 0], dtype=np.int64), terms=terms, e_t=np.zeros(0), e_r=np.zeros(0),
               margins=np.zeros(2), scale=np.ones(2))
    if n == 0:
        return res
    i, k, a, b = terms.T
    poses = [c["est_pos"][i], c["est_pos"][k], c["gt_pos"][a], c["gt_pos"][b]], [c["est_rot"][i], c["est_rot"][k], c["gt_rot"][a], c["gt_rot"][b]]
    for q, group in enumerate(poses):
        v = np.abs(np.concatenate([x.ravel() for x in group]))
        v = v[np.isfinite(v)]
        res["scale"][q] = max(1.0, float(v.max())) if v.size else 1.0
    if not all(np.isfinite(x).all() for group in poses for x in group):
        res["counts"][2] = 1
        return res
    M = lambda x: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(x).reshape(3, -1)])   # noqa: E731
    V = lambda x: mp.matrix([mp.mpf(float(v)) for v in x])                                                 # noqa: E731
    e_t, e_r = [], []
    for i_, k_, a_, b_ in terms:
        Ri, Rk, Qa, Qb = M(c["est_rot"][i_]), M(c["est_rot"][k_]), M(c["gt_rot"][a_]), M(c["gt_rot"][b_])
        dRe, dpe = Ri.T * Rk, Ri.T * (V(c["est_pos"][k_]) - V(c["est_pos"][i_]))
        dRg, dpg = Qa.T * Qb, Qa.T * (V(c["gt_pos"][b_]) - V(c["gt_pos"][a_]))
        d = dpe - dpg
        E = dRg.T * dRe
        s = mp.sqrt((E[2, 1] - E[1, 2]) ** 2 + (E[0, 2] - E[2, 0]) ** 2 + (E[1, 0] - E[0, 1]) ** 2) / 2
        cc = (E[0, 0] + E[1, 1] + E[2, 2] - 1) / 2
        e_t.append(mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2))
        e_r.append(mp.atan2(s, cc))
    for q, e in enumerate((e_t, e_r)):
        order = sorted(range(n), key=lambda x: (-e[x], x))
        res["figures"][3 * q:3 * q + 3] = [float(mp.sqrt(mp.fsum(x * x for x in e) / n)), float(mp.fsum(e) / n), float(e[order[0]])]
        res["counts"][3 + q] = int(terms[order[0], 0])
        res["margins"][q] = float(e[order[0]] - e[order[1]]) if n > 1 else float("inf")
    res["e_t"], res["e_r"] = np.array([float(x) for x in e_t]), np.array([float(x) for x in e_r])
    return res


def evaluate(cases):
    """{key: array}: per case and mode `name/m<q>/<field>`."""
    import mpmath as mp

    mp.mp.dps = 50
    out = {}
    for name, c in cases.items():
        for q, delta, flags in rc.modes(c):
            for f, v in evaluate_mode(c, delta, flags, mp).items():
                out[f"{name}/m{q}/{f}"] = v
    return out


def check_worst(cases, out):
    """What tests/rpecases.py says about the worst terms, asserted."""
    for name, c in cases.items():
        for q, _, _ in rc.modes(c):
            k = f"{name}/m{q}/"
            cnt, mar, sc = out[k + "counts"], out[k + "margins"], out[k + "scale"]
            if cnt[0] < 2 or cnt[2]:
                continue
            tols = (rc.tol_t(sc[0]), rc.tol_r(sc[1]))
            if name in rc.TIES:
                assert tuple(cnt[3:5]) == (out[k + "terms"][0, 0],) * 2, (name, q, "a tie case whose worst is not its first term")
            elif name in rc.RIGID:
                assert out[k + "e_t"].max() <= 4 * tols[0] and out[k + "e_r"].max() <= 4 * tols[1], (name, q, "a rigid case with a term above 4 tol")
            else:
                assert mar[0] > 4 * tols[0] and mar[1] > 4 * tols[1], (name, q, mar, tols, "worst term not separated from the runner-up")


def numpy_ratios(cases, out):
    """Worst |x_numpy - x_50| / (2^-53 S) and / (2^-53 M^2) over figures and term values, with where."""
    from legkilo_amd import tum

    worst = [(0.0, None), (0.0, None)]
    for name, c in cases.items():
        for q, delta, flags in rc.modes(c):
            k = f"{name}/m{q}/"
            got = tum.rpe(c["est_t"], c["est_pos"], c["est_rot"], c["gt_t"], c["gt_pos"], c["gt_rot"], c["max_dt"], delta, by_index=bool(flags))
            assert np.array_equal(got["terms"], out[k + "terms"]), (name, q)
            if out[k + "counts"][0] == 0 or out[k + "counts"][2]:
                continue
            sc = out[k + "scale"]
            for h, (e, unit) in enumerate((("e_t", rc.ULP * sc[0]), ("e_r", rc.ULP * sc[1] ** 2))):
                d = max(float(np.abs(got[e] - out[k + e]).max()), max(abs(got[f] - out[k + "figures"][3 * h + g]) for g, f in enumerate(rc.FIGURES[3 * h:3 * h + 3])))
                if d / unit > worst[h][0]:
                    worst[h] = (d / unit, (name, q))
    return worst


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lk_pkg  # noqa: E402

    lk_pkg.load()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "rpe_cases.npz")
    cases = rc.build()
    out = {}
    for name, c in cases.items():
        for k in rc.KEYS:
            out[f"{name}/in/{k}"] = c[k]
        out[f"{name}/in/max_dt"] = np.array([c["max_dt"]])
        out[f"{name}/in/modes"] = c["modes"]
    ev = evaluate(cases)
    (rt, wt), (rr, wr) = numpy_ratios(cases, ev)
    print(f"numpy restatement: NUMPY_RATIO_T {rt:.3f} at {wt}, NUMPY_RATIO_R {rr:.3f} at {wr}")
    check_worst(cases, ev)
    out.update(ev)
    np.savez_compressed(path, **rc.pack(out))
    print("wrote", path, os.path.getsize(path), "bytes")
