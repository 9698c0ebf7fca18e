"""Writes tests/golden/ate_cases.npz: the inputs of every case of tests/atecases.py as build() gives them here (`names`, `name/in/...`), and each
case, with and without alignment, evaluated at 50 digits (mpmath) and rounded to float64 (`name/a<flag>/...`).  The pairs are those of the header's association rule (exact arithmetic on the float64 stamps); the
alignment is the SVD solution with the det = +1 correction (mp.svd_r), the figures are rmse, mean and max of e_i = |g_i - (R p_i + t)|, the worst
pair's estimate index and the margin by which it leads the runner-up.

    python tests/golden/make_ate_cases.py [out.npz]

The figures are a function of the frozen inputs alone: tests/test_ate_host.py runs evaluate() on them again and compares bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import atecases  # noqa: E402

FIGURES = ("rmse", "mean", "max")


def pairs_exact(c):
    """The header's association in exact arithmetic on the stamps, but for the one rounded subtraction the rule itself is stated in."""
    out = []
    gt = c["gt_t"]
    if len(gt):
        for i, te in enumerate(c["est_t"]):
            d = np.abs(te - gt)                  # "one double subtraction": the rule is about this float64 value
            j = int(np.argmin(d))
            if d[j] <= c["max_dt"]:
                out.append((i, j))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def evaluate_case(c, flag, mp):
    pairs = pairs_exact(c)
    nan = float("nan")
    res = dict(n_pairs=len(pairs), status=0, rmse=nan, mean=nan, max=nan, worst=0, worst_margin=0.0, pairs=pairs)
    if len(pairs) == 0:
        return res
    g64, p64 = c["gt_pos"][pairs[:, 1]], c["est_pos"][pairs[:, 0]]
    if not (np.isfinite(g64).all() and np.isfinite(p64).all()):
        res["status"] = 1
        return res
    n = len(pairs)
    g = mp.matrix([[mp.mpf(float(v)) for v in row] for row in g64])
    p = mp.matrix([[mp.mpf(float(v)) for v in row] for row in p64])
    if flag:
        cg = [mp.fsum(g[i, k] for i in range(n)) / n for k in range(3)]
        cp = [mp.fsum(p[i, k] for i in range(n)) / n for k in range(3)]
        H = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                H[a, b] = mp.fsum((p[i, a] - cp[a]) * (g[i, b] - cg[b]) for i in range(n))
        U, _, Vt = mp.svd_r(H)
        V = Vt.T
        D = mp.eye(3)
        D[2, 2] = mp.sign(mp.det(V * U.T)) or mp.mpf(1)
        R = V * D * U.T
    else:
        cg = cp = [mp.mpf(0)] * 3
        R = mp.eye(3)
    e = []
    for i in range(n):
        d = [g[i, a] - cg[a] - mp.fsum(R[a, b] * (p[i, b] - cp[b]) for b in range(3)) for a in range(3)]
        e.append(mp.sqrt(mp.fsum(x * x for x in d)))
    order = sorted(range(n), key=lambda i: (-e[i], i))
    res.update(rmse=float(mp.sqrt(mp.fsum(x * x for x in e) / n)), mean=float(mp.fsum(e) / n), max=float(e[order[0]]),
               worst=int(pairs[order[0], 0]), worst_margin=float(e[order[0]] - e[order[1]]) if n > 1 else float("inf"))
    return res


def evaluate(cases):
    """{key: array}: per case and flag `name/a<flag>/<field>`."""
    import mpmath as mp

    mp.mp.dps = 50
    out = {}
    for name in cases:
        for flag in atecases.FLAGS:
            r = evaluate_case(cases[name], flag, mp)
            k = f"{name}/a{flag}/"
            out[k + "figures"] = np.array([r[f] for f in FIGURES], dtype=np.float64)
            out[k + "counts"] = np.array([r["n_pairs"], r["status"], r["worst"]], dtype=np.int64)
            out[k + "worst_margin"] = np.array([r["worst_margin"]], dtype=np.float64)
            out[k + "pairs"] = r["pairs"]
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ate_cases.npz")
    cases = atecases.build()
    out = {"names": np.array(list(cases))}
    for name, c in cases.items():
        for k in atecases.KEYS:
            out[f"{name}/in/{k}"] = c[k]
        out[f"{name}/in/max_dt"] = np.array([c["max_dt"]])
    out.update(evaluate(cases))
    np.savez_compressed(path, **out)
    print("wrote", path)
