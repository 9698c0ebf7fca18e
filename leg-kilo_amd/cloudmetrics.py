"""Map-cloud metrics on the host: the float64 numpy statement of lk_clouds_c2c_dev's definition (include/legkilo_hip.h) and the F-score built
on its records.  Brute force in blocks - the reference of the tests and of tools/map_c2c.py, not a fast path; touches no device."""
import numpy as np

NO_MATCH = 0xFFFFFFFF
LK_C2C_NONFINITE = 1
LK_C2C_RANGE = 2


def nearest(query, ref, block=2048):
    """(j, d2) of every query point over the WHOLE reference cloud, no reach applied: d2 = (dx*dx + dy*dy) + dz*dz in float64 from the float32
    coordinates, j the smallest index among the minimisers.  query [n, >= 3], ref [m, >= 3]; m == 0 gives j = NO_MATCH, d2 = inf."""
    q = np.asarray(query, dtype=np.float32)[:, :3].astype(np.float64)
    r = np.asarray(ref, dtype=np.float32)[:, :3].astype(np.float64)
    j = np.full(len(q), NO_MATCH, dtype=np.uint32)
    d2 = np.full(len(q), np.inf)
    if len(r) == 0:
        return j, d2
    block = max(1, min(block, (1 << 21) // len(r)))   # (a block's difference array stays near 50 MB)
    for a in range(0, len(q), block):
        d = q[a:a + block, None, :] - r[None, :, :]
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        k = np.argmin(s, axis=1)                      # (the first of equal minima)
        j[a:a + block], d2[a:a + block] = k, s[np.arange(len(k)), k]
    return j, d2


def status(query, ref, max_dist):
    """The status bits of a pair: LK_C2C_NONFINITE for a non-finite coordinate in either cloud, LK_C2C_RANGE for |p / max_dist| >= 2^30."""
    st = 0
    for c in (query, ref):
        p = np.asarray(c, dtype=np.float32)[:, :3].astype(np.float64)
        fin = np.isfinite(p)
        if not fin.all():
            st |= LK_C2C_NONFINITE
        if (np.abs(p[fin] / max_dist) >= 2.0 ** 30).any():
            st |= LK_C2C_RANGE
    return st


def c2c(query, ref, max_dist, thr=()):
    """Cloud-to-cloud distance of one pair as lk_clouds_c2c_dev defines it.  Returns a dict: j uint32 [n] and d2 float64 [n] (NO_MATCH / inf where
    the point is unmatched), matched bool [n], rmse, mean, max, n_query, n_matched, n_within (one count per threshold), worst, status."""
    n = len(query)
    thr = [float(t) for t in thr]
    st = status(query, ref, max_dist)
    out = dict(j=np.full(n, NO_MATCH, dtype=np.uint32), d2=np.full(n, np.inf), matched=np.zeros(n, dtype=bool), rmse=np.nan, mean=np.nan, max=np.nan,
               n_query=n, n_matched=0, n_within=[0] * len(thr), worst=0, status=st)
    if st:
        return out
    j, d2 = nearest(query, ref)
    m = d2 <= max_dist * max_dist
    out["matched"] = m
    out["j"][m], out["d2"][m] = j[m], d2[m]
    if m.any():
        v = d2[m]
        out.update(rmse=float(np.sqrt(v.sum() / len(v))), mean=float(np.sqrt(v).sum() / len(v)), max=float(np.sqrt(v.max())), n_matched=int(len(v)),
                   n_within=[int((v <= t * t).sum()) for t in thr], worst=int(np.flatnonzero(m)[np.argmax(v)]))
    return out


def fscore(acc_rec, comp_rec, k):
    """(precision, recall, F) at threshold k from the records of the two directions: acc_rec - the map as query against the survey, comp_rec - the
    survey as query against the map (lk_c2c records, or c2c's dicts).  precision = n_within[k] / n_query of the first, recall the same of the
    second, F their harmonic mean; an empty query cloud gives 0, and F is 0 when both are."""
    def frac(rec):
        n = int(rec["n_query"])
        return float(int(rec["n_within"][k])) / n if n else 0.0
    p, r = frac(acc_rec), frac(comp_rec)
    return p, r, (2.0 * p * r / (p + r) if p + r > 0.0 else 0.0)
