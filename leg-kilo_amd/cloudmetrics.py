"""Map-cloud metrics on the host: the float64 numpy statements of lk_clouds_c2c_dev's and lk_clouds_mme_dev's definitions (include/legkilo_hip.h)
and the F-score built on the former's records.  Brute force in blocks - the reference of the tests and of tools/map_c2c.py / map_mme.py, not a fast
path; touches no device."""
import numpy as np

NO_MATCH = 0xFFFFFFFF
LK_C2C_NONFINITE = 1
LK_C2C_RANGE = 2
LK_MME_NONFINITE = 1
LK_MME_RANGE = 2
MME_SPARSE, MME_FLAT, MME_SCORED = 0, 1, 2
MME_FLOOR = 2.0 ** -30
LN_2PIE_3 = 8.5136311992280364508   # 3 ln(2 pi e)


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


def mme_moments(cloud, radius, block=1024):
    """(n, s [n, 3], M [n, 6]) of every point of a cloud as lk_clouds_mme_dev defines them: the records within `radius` (d2 <= radius * radius, the
    point itself among them) and the sums of their offsets u = p_j - p_i about the point and of u u^T (xx xy xz yy yz zz), in index order."""
    p = np.asarray(cloud, dtype=np.float32)[:, :3].astype(np.float64)
    m = len(p)
    n, s, mm = np.zeros(m, dtype=np.uint32), np.zeros((m, 3)), np.zeros((m, 6))
    if m == 0:
        return n, s, mm
    r2 = radius * radius
    block = max(1, min(block, (1 << 21) // m))
    for a in range(0, m, block):
        d = p[a:a + block, None, :] - p[None, :, :]                     # q - r, as d2 is stated
        inside = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= r2
        u = np.where(inside[..., None], -d, 0.0)                        # (negation is exact)
        n[a:a + block] = inside.sum(axis=1)
        s[a:a + block] = np.cumsum(u, axis=1)[:, -1, :]                 # (cumsum: one term after the other, no pairwise tree)
        for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            mm[a:a + block, k] = np.cumsum(u[..., i] * u[..., j], axis=1)[:, -1]
    return n, s, mm


def mme_status(cloud, radius):
    p = np.asarray(cloud, dtype=np.float32)[:, :3].astype(np.float64)
    fin = np.isfinite(p)
    return (0 if fin.all() else LK_MME_NONFINITE) | (LK_MME_RANGE if (np.abs(p[fin] / radius) >= 2.0 ** 30).any() else 0)


def mme(cloud, radius, min_pts=5):
    """Mean map entropy and mean plane variance of one cloud as lk_clouds_mme_dev defines them.  Returns a dict: n uint32 [m], cls uint8 [m]
    (MME_SPARSE / MME_FLAT / MME_SCORED), dense / flat / scored bool [m], h and lmin float64 [m] (NaN where the point has none), and the record
    fields mme, mpv, h_max, n_points, n_dense, n_scored, n_pairs, worst, status."""
    m = len(cloud)
    st = mme_status(cloud, radius)
    nan = np.full(m, np.nan)
    out = dict(n=np.zeros(m, dtype=np.uint32), cls=np.zeros(m, dtype=np.uint8), h=nan.copy(), lmin=nan.copy(), mme=np.nan, mpv=np.nan, h_max=np.nan,
               n_points=m, n_dense=0, n_scored=0, n_pairs=0, worst=0, status=st)
    if not st and m:
        n, s, mm = mme_moments(cloud, radius)
        dense = n >= min_pts
        nn = n[dense].astype(np.float64)
        sd, md = s[dense], mm[dense]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        c = np.stack([(md[:, k] - sd[:, i] * sd[:, j] / nn) / (nn - 1.0) for k, (i, j) in enumerate(pairs)], axis=1) if dense.any() else np.zeros((0, 6))
        tr = (c[:, 0] + c[:, 3]) + c[:, 5]
        det = (c[:, 0] * (c[:, 3] * c[:, 5] - c[:, 4] * c[:, 4]) - c[:, 1] * (c[:, 1] * c[:, 5] - c[:, 4] * c[:, 2])) + c[:, 2] * (c[:, 1] * c[:, 4] - c[:, 3] * c[:, 2])
        t = tr / 3.0
        flat = det <= MME_FLOOR * ((t * t) * t)
        full = np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], axis=1).reshape(-1, 3, 3)
        lmin = np.maximum(0.0, np.linalg.eigvalsh(full)[:, 0]) if len(full) else np.zeros(0)
        h = np.full(len(det), np.nan)
        h[~flat] = 0.5 * (LN_2PIE_3 + np.log(det[~flat]))
        di = np.flatnonzero(dense)
        out["n"] = n
        out["cls"][di] = np.where(flat, MME_FLAT, MME_SCORED)
        out["h"][di], out["lmin"][di] = h, lmin
        sc = np.flatnonzero(out["cls"] == MME_SCORED)
        out.update(n_dense=int(dense.sum()), n_scored=int(len(sc)), n_pairs=int(n.astype(np.uint64).sum()))
        if len(di):
            out["mpv"] = float(lmin.sum() / len(di))
        if len(sc):
            hs = out["h"][sc]
            out.update(mme=float(hs.sum() / len(sc)), h_max=float(hs.max()), worst=int(sc[np.argmax(hs)]))
    out["dense"], out["flat"], out["scored"] = out["cls"] != MME_SPARSE, out["cls"] == MME_FLAT, out["cls"] == MME_SCORED
    return out
