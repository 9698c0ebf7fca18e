"""float64 numpy restatement of lk_traj_ate_dev (include/legkilo_hip.h): the association as the header defines it, tum.ate for the error, and mean /
max / worst beside it from the same aligned differences.  `variant` names a deliberately WRONG restatement (tests/test_ate_host.py shows that each
one fails on a named case of tests/atecases.py): "no_det" - the SVD solution without the det = +1 correction; "one_pass" - the cross-covariance as
sum x y^T - n mean mean^T; "strict" - a pair counts for |dt| < max_dt; "later" - the later sample wins on equal distance."""
import numpy as np

from legkilo_amd import tum

NONFINITE = 1


def associate(est_t, gt_t, max_dt, variant=None):
    """[(i, j)] int64 [k, 2]: j = the ground-truth sample that minimises fabs(est_t[i] - gt_t[j]), the earliest on equal distance; kept for <= max_dt."""
    out = []
    if len(gt_t):
        for i, te in enumerate(est_t):
            d = np.abs(te - gt_t)
            j = int(np.argmin(d)) if variant != "later" else int(np.flatnonzero(d == d.min())[-1])
            if (d[j] < max_dt) if variant == "strict" else (d[j] <= max_dt):
                out.append((i, j))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def align(g, p, variant=None):
    """tum.ate's alignment (pa = g, pb = p): R, t with g ~ R p + t."""
    cg, cp = g.mean(0), p.mean(0)
    if variant == "one_pass":
        H = p.T @ g - len(g) * np.outer(cp, cg)
    else:
        H = (p - cp).T @ (g - cg)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, 1.0 if variant == "no_det" else np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cg, cp


def ate(c, flag, variant=None):
    """One case of atecases.CASES -> dict(pairs, n_pairs, status, rmse, mean, max, worst, e)."""
    pairs = associate(c["est_t"], c["gt_t"], c["max_dt"], variant)
    res = dict(pairs=pairs, n_pairs=len(pairs), status=0, rmse=np.nan, mean=np.nan, max=np.nan, worst=0, e=np.zeros(0))
    if len(pairs) == 0:
        return res
    g, p = c["gt_pos"][pairs[:, 1]], c["est_pos"][pairs[:, 0]]
    if not (np.isfinite(g).all() and np.isfinite(p).all()):
        res["status"] = NONFINITE
        return res
    if flag:
        R, cg, cp = align(g, p, variant)
        d = g - ((p - cp) @ R.T + cg)          # tum.ate's own expression
        rmse = tum.ate(g, p, align=True) if variant is None else float(np.sqrt((d * d).sum(1).mean()))
    else:
        d = g - p
        rmse = tum.ate(g, p, align=False)
    e = np.sqrt((d * d).sum(1))
    res.update(rmse=rmse, mean=float(e.mean()), max=float(e.max()), worst=int(pairs[int(np.argmax(e)), 0]), e=e)
    return res
