"""Map-cloud metrics on the host: the float64 numpy statements of the definitions of lk_clouds_c2c_dev, lk_clouds_align_dev,
lk_clouds_align_plane_dev, lk_clouds_normals_dev, lk_clouds_mme_dev, lk_clouds_sor_dev, lk_clouds_cluster_dev and lk_clouds_planes_dev (include/legkilo_hip.h) and the F-score built on the first one's records.  Brute force in blocks - the reference of the tests and of tools/map_c2c.py / map_mme.py, not a fast
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


LK_ALIGN_NONFINITE, LK_ALIGN_RANGE, LK_ALIGN_FEW, LK_ALIGN_CONVERGED, LK_ALIGN_BAD_T0 = 1, 2, 4, 8, 16


def move(cloud, T):
    """The float64 moved points [n, 3] of lk_clouds_align_dev: m = ((R[a,0] x + R[a,1] y) + R[a,2] z) + t[a] from the float32 coordinates; T = 12
    doubles, R row-major then t."""
    p = np.asarray(cloud, dtype=np.float32)[:, :3].astype(np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(12)
    return np.stack([((T[3 * a] * p[:, 0] + T[3 * a + 1] * p[:, 1]) + T[3 * a + 2] * p[:, 2]) + T[9 + a] for a in range(3)], axis=1)


def transform(cloud, T):
    """lk_clouds_transform_dev's statement for one cloud of x y z w records: the moved points rounded once to float32, w kept bit for bit."""
    rec = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
    out = rec.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, :3] = move(rec, T).astype(np.float32)
    out[:, 3].view(np.uint32)[:] = rec[:, 3].view(np.uint32)
    return out


def nearest_moved(moved, ref, max_dist, block=2048):
    """(j, d2, matched) of float64 moved points [n, 3] over the whole float32 reference cloud by brute force, as lk_clouds_align_dev's search under
    T: a point that is not finite or has |m / max_dist| >= 2^30 is unmatched; j = NO_MATCH and d2 = inf where unmatched.  (By brute force the
    guard changes nothing - a float32 reference point in range lies 64 max_dist or more inside the bound - it is stated because the definition
    states it; what it protects is the cell arithmetic of the grid search.)"""
    m = np.asarray(moved, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(ref, dtype=np.float32)[:, :3].astype(np.float64)
    j = np.full(len(m), NO_MATCH, dtype=np.uint32)
    d2 = np.full(len(m), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(m / max_dist) < 2.0 ** 30).all(axis=1)
    if len(r) and ok.any():
        idx = np.flatnonzero(ok)
        block = max(1, min(block, (1 << 21) // len(r)))
        for a in range(0, len(idx), block):
            sel = idx[a:a + block]
            d = m[sel, None, :] - r[None, :, :]
            s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            k = np.argmin(s, axis=1)
            j[sel], d2[sel] = k, s[np.arange(len(k)), k]
    matched = d2 <= max_dist * max_dist
    j[~matched], d2[~matched] = NO_MATCH, np.inf
    return j, d2, matched


def horn_rotation(S):
    """The proper rotation of Horn's closed form for the centred cross-covariance S [3, 3] (S[a, b] = sum p_a r_b): the unit quaternion that is
    the eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix N, through numpy.linalg.eigh."""
    S = np.asarray(S, dtype=np.float64).reshape(3, 3)
    if not np.isfinite(S).all() or not np.abs(S).max() > 0.0:
        return np.eye(3)
    S = S / np.abs(S).max()
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    n = np.sqrt((w * w + x * x) + (y * y + z * z))
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[(w * w + x * x) - (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), (w * w + y * y) - (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), (w * w + z * z) - (x * x + y * y)]])


def align_step(T, Tn, pbar):
    """(step_rot, step_trans) from T to Tn (12 doubles each) as lk_clouds_align_dev states them: the angle of R' R^T in the atan2 form, and the
    distance the query centroid pbar moves."""
    R, Rn = np.asarray(T[:9]).reshape(3, 3), np.asarray(Tn[:9]).reshape(3, 3)
    E = np.array([[(Rn[i, 0] * R[j, 0] + Rn[i, 1] * R[j, 1]) + Rn[i, 2] * R[j, 2] for j in range(3)] for i in range(3)])
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    s, c = 0.5 * np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), 0.5 * (((E[0, 0] + E[1, 1]) + E[2, 2]) - 1.0)
    mv = lambda X: np.array([((X[3 * a] * pbar[0] + X[3 * a + 1] * pbar[1]) + X[3 * a + 2] * pbar[2]) + X[9 + a] for a in range(3)])   # noqa: E731
    d = mv(Tn) - mv(T)
    return float(np.arctan2(s, c)), float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def align(query, ref, max_dist, T0=None, max_iter=30, eps_rot=1e-6, eps_trans=1e-6, thr=(), variant=None):
    """Rigid alignment of one pair as lk_clouds_align_dev defines it: search under T by brute force on the float64 moved points, Horn's solve from
    the original points of the matched pairs, until a solve moves by no more than both eps or max_iter solves are taken.  Returns a dict: T [12]
    (R row-major, then t), iters, status, rmse_first, n_matched_first, step_rot, step_trans, first = (j, matched) of the first search, and c2c -
    the final search as c2c's dict (j, d2, matched, rmse, mean, max, n_query, n_matched, n_within, worst, status).
    variant (test aid): one of the wrong restatements tests/test_align_host.py expects to fail - "compose", "reflect", "all_n", "one_eps"."""
    q, r = np.asarray(query, dtype=np.float32)[:, :3], np.asarray(ref, dtype=np.float32)[:, :3]
    n = len(q)
    thr = [float(t) for t in thr]
    T = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]) if T0 is None else np.asarray(T0, dtype=np.float64).reshape(12).copy()
    st = status(q, r, max_dist) | (0 if np.isfinite(T).all() else LK_ALIGN_BAD_T0)
    none = dict(j=np.full(n, NO_MATCH, dtype=np.uint32), d2=np.full(n, np.inf), matched=np.zeros(n, dtype=bool), rmse=np.nan, mean=np.nan, max=np.nan,
                n_query=n, n_matched=0, n_within=[0] * len(thr), worst=0, status=st & 3)
    out = dict(T=T, iters=0, status=st, rmse_first=np.nan, n_matched_first=0, step_rot=np.nan, step_trans=np.nan, first=(none["j"], none["matched"]), c2c=none)
    if st:
        return out
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    iters, stopped, first = 0, False, None
    while True:
        j, d2, m = nearest_moved(move(q, T), r, max_dist)
        if first is None:
            first = (j.copy(), m.copy())
            out.update(n_matched_first=int(m.sum()), rmse_first=float(np.sqrt(d2[m].sum() / m.sum())) if m.any() else np.nan, first=first)
        if iters == max_iter or stopped:
            break
        if m.sum() < 3:
            st |= LK_ALIGN_FEW
            break
        P, G = q64[m], r64[j[m]]
        cnt = n if variant == "all_n" else len(P)
        pbar, rbar = P.sum(axis=0) / cnt, G.sum(axis=0) / cnt
        if variant == "compose":      # the solve from the MOVED points, composed onto T, about the origin instead of the centroids
            Pm = move(q[m], T)
            Rd = horn_rotation(Pm.T @ G)
            td = rbar - Rd @ (Pm.sum(axis=0) / cnt)
            Rn = Rd @ T[:9].reshape(3, 3)
            Tn = np.r_[Rn.reshape(9), Rd @ T[9:] + td]
        else:
            S = (P - pbar).T @ (G - rbar)
            if variant == "reflect":  # SVD without the determinant fix
                U, _, Vt = np.linalg.svd(S)
                Rn = Vt.T @ U.T
            else:
                Rn = horn_rotation(S)
            Tn = np.r_[Rn.reshape(9), rbar - np.array([(Rn[a, 0] * pbar[0] + Rn[a, 1] * pbar[1]) + Rn[a, 2] * pbar[2] for a in range(3)])]
        step_rot, step_trans = align_step(T, Tn, pbar)
        T, iters = Tn, iters + 1
        out.update(step_rot=step_rot, step_trans=step_trans)
        if step_rot <= eps_rot and (variant == "one_eps" or step_trans <= eps_trans):
            st |= LK_ALIGN_CONVERGED
            stopped = True
    fin = dict(none, status=0)
    fin.update(j=j, d2=d2, matched=m)
    if m.any():
        v = d2[m]
        fin.update(rmse=float(np.sqrt(v.sum() / len(v))), mean=float(np.sqrt(v).sum() / len(v)), max=float(np.sqrt(v.max())), n_matched=int(len(v)),
                   n_within=[int((v <= t * t).sum()) for t in thr], worst=int(np.flatnonzero(m)[np.argmax(v)]))
    out.update(T=T, iters=iters, status=st, c2c=fin)
    return out


LK_ALIGN_DEGENERATE = 32
PLANE_MIN_USED = 6
PLANE_PIVOT = 2.0 ** -20


def quat_to_rot(w, x, y, z):
    return np.array([[(w * w + x * x) - (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), (w * w + y * y) - (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), (w * w + z * z) - (x * x + y * y)]])


def nearest_rotation(R1):
    """The proper rotation nearest R1 [3, 3] as lk_clouds_align_plane_dev takes it: Horn's closed form on R1 TRANSPOSED (S[a, b] = sum p_a g_b with
    g = R p and sum p p^T = 1 is R^T), which returns a rotation as itself."""
    return horn_rotation(np.asarray(R1, dtype=np.float64).reshape(3, 3).T)


def plane_solve(H, g, scale=True):
    """x = -D (D H D)^-1 D g by Cholesky in natural order without pivoting, D = diag(H)^(-1/2); None for a diagonal entry <= 0 or a pivot <= 2^-20
    (an unobserved direction).  scale False (test aid): no D, the pivot test on H itself."""
    H, g = np.asarray(H, dtype=np.float64).reshape(6, 6), np.asarray(g, dtype=np.float64).reshape(6)
    dg = np.diag(H)
    if not (dg > 0.0).all():
        return None
    d = 1.0 / np.sqrt(dg) if scale else np.ones(6)
    A = (H * d[:, None]) * d[None, :]
    L = np.zeros((6, 6))
    for j in range(6):
        s = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not s > PLANE_PIVOT:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (d[i] * g[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    for i in range(5, -1, -1):
        y[i] = (y[i] - (L[i + 1:, i] * y[i + 1:]).sum()) / L[i, i]
    return -(d * y)


def align_plane(query, ref, ref_normals, max_dist, T0=None, max_iter=30, eps_rot=1e-6, eps_trans=1e-6, thr=(), variant=None):
    """Point-to-plane alignment of one pair as lk_clouds_align_plane_dev defines it: align's search (the normals play no part in it), then over the
    matched points whose reference normal is finite the 6 x 6 normal equations about the moved centroid, the scaled Cholesky solve, the rotation
    about that centroid composed onto T and re-orthonormalised.  ref_normals [m, >= 3] float32, used as given.  Returns align's dict and
    rmse_plane_first, rmse_plane, n_used_first, n_used.
    variant (test aid): one of the wrong restatements tests/test_plane_host.py expects to fail - "origin", "no_scale", "unit_normals",
    "count_invalid", "no_ortho"."""
    q, r = np.asarray(query, dtype=np.float32)[:, :3], np.asarray(ref, dtype=np.float32)[:, :3]
    nr = np.asarray(ref_normals, dtype=np.float32)
    nr = nr.reshape(-1, nr.shape[-1] if nr.ndim == 2 else 4)[:, :3].astype(np.float64)
    n = len(q)
    thr = [float(t) for t in thr]
    T = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]) if T0 is None else np.asarray(T0, dtype=np.float64).reshape(12).copy()
    st = status(q, r, max_dist) | (0 if np.isfinite(T).all() else LK_ALIGN_BAD_T0)
    none = dict(j=np.full(n, NO_MATCH, dtype=np.uint32), d2=np.full(n, np.inf), matched=np.zeros(n, dtype=bool), rmse=np.nan, mean=np.nan, max=np.nan,
                n_query=n, n_matched=0, n_within=[0] * len(thr), worst=0, status=st & 3)
    out = dict(T=T, iters=0, status=st, rmse_first=np.nan, n_matched_first=0, step_rot=np.nan, step_trans=np.nan, first=(none["j"], none["matched"]), c2c=none,
               rmse_plane_first=np.nan, rmse_plane=np.nan, n_used_first=0, n_used=0)
    if st:
        return out
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    fin = np.isfinite(nr).all(axis=1) if len(nr) else np.zeros(0, dtype=bool)
    if variant == "unit_normals":
        with np.errstate(invalid="ignore", divide="ignore"):
            nr = nr / np.sqrt((nr * nr).sum(axis=1))[:, None]
    iters, stopped, first = 0, False, None
    while True:
        moved = move(q, T)
        j, d2, m = nearest_moved(moved, r, max_dist)
        u = m.copy()
        u[m] = fin[j[m]]
        cnt = int(m.sum()) if variant == "count_invalid" else int(u.sum())
        Mv, G, Nn, P = moved[u], r64[j[u]], nr[j[u]], q64[u]
        D = Mv - G
        e = (Nn[:, 0] * D[:, 0] + Nn[:, 1] * D[:, 1]) + Nn[:, 2] * D[:, 2]
        rp = float(np.sqrt((e * e).sum() / cnt)) if cnt else np.nan
        if first is None:
            first = (j.copy(), m.copy())
            out.update(n_matched_first=int(m.sum()), rmse_first=float(np.sqrt(d2[m].sum() / m.sum())) if m.any() else np.nan, first=first, rmse_plane_first=rp,
                       n_used_first=cnt)
        out.update(rmse_plane=rp, n_used=cnt)
        if iters == max_iter or stopped:
            break
        if cnt < PLANE_MIN_USED:
            st |= LK_ALIGN_FEW
            break
        mbar, pbar = Mv.sum(axis=0) / cnt, P.sum(axis=0) / cnt
        about = np.zeros(3) if variant == "origin" else mbar
        Cc = Mv - about
        A = np.concatenate([np.cross(Cc, Nn), Nn], axis=1)
        x = plane_solve(A.T @ A, A.T @ e, scale=variant != "no_scale")
        if x is None:
            st |= LK_ALIGN_DEGENERATE
            break
        if variant == "origin":       # (the same step in exact arithmetic: v about mbar = v about the origin + omega x mbar)
            x = np.r_[x[:3], x[3:] + np.cross(x[:3], mbar)]
        theta = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        dR = np.eye(3) if theta == 0.0 else quat_to_rot(np.cos(theta / 2.0), np.sin(theta / 2.0) * x[0] / theta, np.sin(theta / 2.0) * x[1] / theta,
                                                        np.sin(theta / 2.0) * x[2] / theta)
        R1 = dR @ T[:9].reshape(3, 3)
        Rn = R1 if variant == "no_ortho" else nearest_rotation(R1)
        Tn = np.r_[Rn.reshape(9), dR @ (T[9:] - mbar) + (mbar + x[3:])]
        step_rot, step_trans = align_step(T, Tn, pbar)
        T, iters = Tn, iters + 1
        out.update(step_rot=step_rot, step_trans=step_trans)
        if step_rot <= eps_rot and step_trans <= eps_trans:
            st |= LK_ALIGN_CONVERGED
            stopped = True
    fin_rec = dict(none, status=0)
    fin_rec.update(j=j, d2=d2, matched=m)
    if m.any():
        v = d2[m]
        fin_rec.update(rmse=float(np.sqrt(v.sum() / len(v))), mean=float(np.sqrt(v).sum() / len(v)), max=float(np.sqrt(v.max())), n_matched=int(len(v)),
                       n_within=[int((v <= t * t).sum()) for t in thr], worst=int(np.flatnonzero(m)[np.argmax(v)]))
    out.update(T=T, iters=iters, status=st, c2c=fin_rec)
    return out


def normals(cloud, radius, min_pts=5, min_planarity=0.0, variant=None):
    """Per-point normals of one cloud as lk_clouds_normals_dev defines them: mme's neighbourhoods and covariance, l0 <= l1 <= l2 its eigenvalues,
    planarity w = (l1 - l0) / l2 (0 when l2 <= 0), valid when n_i >= min_pts and w >= min_planarity; the normal is the unit eigenvector of l0 with the
    float64 component of largest magnitude positive (the first on ties), rounded once to float32.  Returns a dict: rec float32 [m, 4] (nx ny nz w;
    NaN in nx ny nz where the point is not valid, in w too where it is sparse), n uint32 [m], w float64 [m], valid / dense bool [m], vec float64
    [m, 3] (the oriented eigenvector of every dense point), n_points, n_valid, status.  variant "sign_f32" (test aid): the sign rule applied to
    the float32 rounding."""
    m = len(cloud)
    st = mme_status(cloud, radius)
    out = dict(rec=np.full((m, 4), np.nan, dtype=np.float32), n=np.zeros(m, dtype=np.uint32), w=np.full(m, np.nan), valid=np.zeros(m, dtype=bool),
               dense=np.zeros(m, dtype=bool), vec=np.full((m, 3), np.nan), n_points=m, n_valid=0, status=st)
    if st or not m:
        return out
    n, s, mm = mme_moments(cloud, radius)
    dense = n >= min_pts
    out["n"], out["dense"] = n, dense
    if not dense.any():
        return out
    nn, sd, md = n[dense].astype(np.float64), s[dense], mm[dense]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    c = np.stack([(md[:, k] - sd[:, i] * sd[:, j] / nn) / (nn - 1.0) for k, (i, j) in enumerate(pairs)], axis=1)
    full = np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], axis=1).reshape(-1, 3, 3)
    ev, V = np.linalg.eigh(full)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(ev[:, 2] > 0.0, (ev[:, 1] - ev[:, 0]) / ev[:, 2], 0.0)
    vec = V[:, :, 0].copy()
    mag = np.abs(vec.astype(np.float32).astype(np.float64)) if variant == "sign_f32" else np.abs(vec)
    lead = vec[np.arange(len(vec)), np.argmax(mag, axis=1)]
    vec[lead < 0.0] *= -1.0
    ok = w >= min_planarity
    di = np.flatnonzero(dense)
    out["w"][di], out["vec"][di], out["valid"][di] = w, vec, ok
    out["rec"][di, 3] = w.astype(np.float32)
    out["rec"][di[ok], :3] = vec[ok].astype(np.float32)
    out["n_valid"] = int(ok.sum())
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


LK_SOR_MAX_K = 32
LK_SOR_NONFINITE = LK_MME_NONFINITE
LK_SOR_RANGE = LK_MME_RANGE


def sor_tree_sum(v):
    """The sum of a cloud's per-point values in lk_sor_stats_kernel's order: lane t of 256 adds the entries t, t + 256, ... one after the other, then
    the partial sums meet in a halving tree.  (Entries that take no part are passed as +0.0, which changes no bit of a sum of non-negative terms.)"""
    v = np.asarray(v, dtype=np.float64)
    rows = np.concatenate([v, np.zeros((-len(v)) % 256)]).reshape(-1, 256)
    part = np.cumsum(rows, axis=0)[-1] if len(rows) else np.zeros(256)
    o = 128
    while o:
        part = part[:o] + part[o:2 * o]
        o >>= 1
    return float(part[0])


def sor(cloud, k, reach, n_sigma, variant=None, block=1024):
    """The statistical outlier filter of one cloud as lk_clouds_sor_dev defines it, by brute force: the candidates of point i are the records j != i
    (by index) with d2 <= reach * reach, cnt_i their number; with cnt_i < k the point is isolated (dbar NaN), else dbar_i is the mean of the roots of
    the k smallest candidate d2, summed in ascending order one after the other; mu and sigma (divisor n_s - 1, 0 for a single point) over the
    non-isolated points, thr = mu + n_sigma * sigma (+inf for n_sigma = inf), kept when dbar_i <= thr.  Returns a dict: keep bool [m], cnt uint32
    [m], dbar float64 [m], src_idx (the kept points' indices), and the record fields mu, sigma, thr, n_points, n_isolated, n_outliers, n_kept, worst,
    status.  variant (test aid, one thing wrong each): "with_self", "self_by_coords", "isolated_in_stats", "biased", "strict_thr", "strict_reach",
    "root_of_mean"."""
    p = np.asarray(cloud, dtype=np.float32)[:, :3].astype(np.float64)
    m, k = len(p), int(k)
    st = mme_status(cloud, reach)
    out = dict(keep=np.zeros(m, dtype=bool), cnt=np.zeros(m, dtype=np.uint32), dbar=np.full(m, np.nan), src_idx=np.zeros(0, dtype=np.uint32), mu=np.nan,
               sigma=np.nan, thr=np.nan, n_points=m, n_isolated=0, n_outliers=0, n_kept=0, worst=0, status=st)
    if st or not m:
        return out
    r2 = reach * reach
    cnt, dbar = out["cnt"], out["dbar"]
    block = max(1, min(block, (1 << 21) // m))
    for a in range(0, m, block):
        d = p[a:a + block, None, :] - p[None, :, :]                     # q - r, as d2 is stated
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        inside = d2 < r2 if variant == "strict_reach" else d2 <= r2
        rows = np.arange(len(d))
        if variant == "self_by_coords":
            inside &= ~(d == 0.0).all(axis=2)
        elif variant != "with_self":
            inside[rows, a + rows] = False
        cnt[a:a + block] = inside.sum(axis=1)
        masked = np.where(inside, d2, np.inf)
        if m < k:
            masked = np.concatenate([masked, np.full((len(d), k - m), np.inf)], axis=1)
        least = np.sort(np.partition(masked, k - 1, axis=1)[:, :k], axis=1)       # the k smallest, ascending
        with np.errstate(invalid="ignore"):
            if variant == "root_of_mean":
                dbar[a:a + block] = np.sqrt(np.cumsum(least, axis=1)[:, -1] / k)
            else:
                dbar[a:a + block] = np.cumsum(np.sqrt(least), axis=1)[:, -1] / k   # (cumsum: one term after the other, no pairwise tree)
    iso = cnt < k
    dbar[iso] = np.nan
    stat = np.where(iso, reach, dbar) if variant == "isolated_in_stats" else dbar
    ok = ~np.isnan(stat)
    n_s = int(ok.sum())
    out["n_isolated"] = int(iso.sum())
    if n_s:
        mu = sor_tree_sum(np.where(ok, stat, 0.0)) / n_s
        e = np.where(ok, stat - mu, 0.0)
        div = n_s if variant == "biased" else n_s - 1
        sigma = float(np.sqrt(sor_tree_sum(e * e) / div)) if n_s > 1 else 0.0
        thr = np.inf if n_sigma == np.inf else mu + n_sigma * sigma
        with np.errstate(invalid="ignore"):
            keep = (dbar < thr) if variant == "strict_thr" else (dbar <= thr)
        out.update(mu=mu, sigma=sigma, thr=float(thr), keep=keep, n_kept=int(keep.sum()), worst=int(np.nanargmax(dbar)) if (~iso).any() else 0)
        out["n_outliers"] = int((~iso).sum()) - out["n_kept"]
    out["src_idx"] = np.flatnonzero(out["keep"]).astype(np.uint32)
    return out


LK_CLUSTER_KEEP_LARGEST = 1
LK_CLUSTER_NONFINITE = LK_MME_NONFINITE
LK_CLUSTER_RANGE = LK_MME_RANGE
LK_CLUSTER_NOISE = 0xFFFFFFFF
CLUSTER_NOISE, CLUSTER_BORDER, CLUSTER_CORE = 0, 1, 2
CLUSTER_VARIANTS = ("border_links", "no_self", "strict_reach", "border_smallest_index", "ids_by_member")


def cluster_pairs(cloud, reach, strict=False, block=1024):
    """Every ordered pair i != j (by index) of a cloud's records with d2 <= reach * reach, by brute force -> (i, j, d2), i ascending."""
    p = np.asfortranarray(np.asarray(cloud, dtype=np.float32)[:, :3].astype(np.float64))
    m = len(p)
    r2 = reach * reach
    ii, jj, dd = [], [], []
    block = max(1, min(block, (1 << 21) // max(m, 1)))
    for a in range(0, m, block):
        dx, dy, dz = (p[a:a + block, None, k] - p[None, :, k] for k in range(3))   # q - r, as d2 is stated
        d2 = (dx * dx + dy * dy) + dz * dz
        inside = d2 < r2 if strict else d2 <= r2
        rows = np.arange(len(dx))
        inside[rows, a + rows] = False
        i, j = np.nonzero(inside)
        ii.append(i + a), jj.append(j), dd.append(d2[i, j])
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dtype=dt)   # noqa: E731
    return cat(ii, np.int64), cat(jj, np.int64), cat(dd, np.float64)


def cluster(cloud, reach, min_pts=1, min_size=0, max_size=0xFFFFFFFF, flags=0, variant=None):
    """DBSCAN of one cloud as lk_clouds_cluster_dev defines it, by brute force with a sequential union-find: n_i = the records within reach, the point
    itself among them; core when n_i >= min_pts; clusters = the connected components of the core points under d2 <= reach * reach; a point that is not
    core joins the cluster of the core point that minimises (d2, index) or is noise; clusters numbered by their smallest core index; kept = in a
    cluster with min_size <= size <= max_size, under LK_CLUSTER_KEEP_LARGEST the largest of those only (the smallest id among equals).  Returns a
    dict: label uint32 [m] (LK_CLUSTER_NOISE for noise), kind uint8 [m], n uint32 [m], cl_size / cl_first uint32 [n_clusters], keep bool [m],
    src_idx, and the record fields n_points, n_core, n_border, n_noise, n_kept, n_clusters, n_kept_clusters, largest, largest_size, status.
    variant (test aid, one thing wrong each): CLUSTER_VARIANTS."""
    m = len(cloud)
    st = mme_status(cloud, reach)
    out = dict(label=np.full(m, LK_CLUSTER_NOISE, dtype=np.uint32), kind=np.zeros(m, dtype=np.uint8), n=np.zeros(m, dtype=np.uint32),
               cl_size=np.zeros(0, dtype=np.uint32), cl_first=np.zeros(0, dtype=np.uint32), keep=np.zeros(m, dtype=bool), src_idx=np.zeros(0, dtype=np.uint32),
               n_points=m, n_core=0, n_border=0, n_noise=0, n_kept=0, n_clusters=0, n_kept_clusters=0, largest=0, largest_size=0, status=st)
    if st or not m:
        return out
    i, j, d2 = cluster_pairs(cloud, reach, strict=variant == "strict_reach")
    n = np.bincount(i, minlength=m).astype(np.uint32) + 1
    core = n - 1 >= min_pts if variant == "no_self" else n >= min_pts
    parent = list(range(m))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    linked = (core[i] | core[j]) if variant == "border_links" else (core[i] & core[j])
    for a, b in zip(i[linked & (j < i)].tolist(), j[linked & (j < i)].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.full(m, -1, dtype=np.int64)
    for v in np.flatnonzero(core).tolist():
        root[v] = find(v)
    if variant == "border_links":   # (a root may then be a border point: name the component by its smallest core member, as the rule says)
        for v in np.flatnonzero(core).tolist():
            root[v] = find(v)
        for r in np.unique(root[core]).tolist():
            root[core & (root == r)] = np.flatnonzero(core & (root == r))[0]
    kind = np.where(core, CLUSTER_CORE, CLUSTER_NOISE).astype(np.uint8)
    cand = ~core[i] & core[j]
    bi, bj, bd = i[cand], j[cand], d2[cand]
    order = np.lexsort((bj, bi)) if variant == "border_smallest_index" else np.lexsort((bj, bd, bi))
    bi, bj = bi[order], bj[order]
    firsts = np.r_[True, bi[1:] != bi[:-1]] if len(bi) else np.zeros(0, dtype=bool)
    root[bi[firsts]] = root[bj[firsts]]
    kind[bi[firsts]] = CLUSTER_BORDER
    member = root >= 0
    roots = np.unique(root[member])                                     # ascending smallest core index: the numbering
    if variant == "ids_by_member" and len(roots):
        roots = roots[np.argsort([np.flatnonzero(root == r)[0] for r in roots], kind="stable")]
    ids = np.full(m, LK_CLUSTER_NOISE, dtype=np.int64)
    lookup = {int(r): k for k, r in enumerate(roots.tolist())}
    ids[member] = [lookup[int(r)] for r in root[member]]
    size = np.bincount(ids[member], minlength=len(roots)).astype(np.uint32)
    ok = (size >= min_size) & (size <= max_size)
    kept_ids = np.flatnonzero(ok)
    if flags & LK_CLUSTER_KEEP_LARGEST and len(kept_ids):
        kept_ids = kept_ids[[int(np.argmax(size[kept_ids]))]]           # (argmax: the first among equals)
    keep = member & np.isin(ids, kept_ids)
    out.update(label=ids.astype(np.uint32), kind=kind, n=n, cl_size=size, cl_first=roots.astype(np.uint32), keep=keep, src_idx=np.flatnonzero(keep).astype(np.uint32),
               n_core=int(core.sum()), n_border=int((kind == CLUSTER_BORDER).sum()), n_noise=int((kind == CLUSTER_NOISE).sum()), n_kept=int(keep.sum()),
               n_clusters=len(roots), n_kept_clusters=len(kept_ids), largest=int(np.argmax(size)) if len(size) else 0, largest_size=int(size.max()) if len(size) else 0)
    return out


def cluster_clouds(clouds, reach, min_pts=1, min_size=0, max_size=0xFFFFFFFF, flags=0, variant=None):
    """cluster() of every cloud of one call -> a list of its dicts.  variant "across_clouds" (test aid): the clouds of the call taken as one cloud and
    the labels cut apart afterwards, so that links cross the clouds' boundaries."""
    if variant != "across_clouds":
        return [cluster(c, reach, min_pts, min_size, max_size, flags, variant) for c in clouds]
    whole = cluster(np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds]), reach, min_pts, min_size, max_size, flags)
    out, at = [], 0
    for c in clouds:
        part = {k: (v[at:at + len(c)] if k in ("label", "kind", "n", "keep") else v) for k, v in whole.items()}
        part["n_points"] = len(c)
        out.append(part)
        at += len(c)
    return out


LK_PLANES_MAX_HYP = 4096
LK_PLANES_MAX_PLANES = 16
LK_PLANES_KEEP_PLANES = 1
LK_PLANES_NONFINITE = LK_MME_NONFINITE
LK_PLANES_RANGE = LK_MME_RANGE
LK_PLANES_NONE = 0xFFFFFFFF
PLANES_GROUP, PLANES_TILE, PLANES_CHUNK = 64, 256, 2048   # lk_planes.h's LK_PLANES_GROUP / _TILE / _CHUNK: where the score kernel's paths change
PLANES_VARIANTS = ("strict", "normalised", "ties_last", "input_indices", "samples_not_counted", "axis_without_aa", "cloud_in_sampler")
_U64 = (1 << 64) - 1


def planes_mix(x):
    """splitmix64 of a uint64 array: the state advanced by the golden gamma, then the finaliser."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def planes_mulhi(u, m):
    """The high 64 bits of u * m for a uint64 array u and 0 <= m < 2^32, in uint64 arithmetic that does not wrap."""
    m, s = np.uint64(m), np.uint64(32)
    return ((u >> s) * m + (((u & np.uint64(0xFFFFFFFF)) * m) >> s)) >> s


def planes_sample(seed, r, h, m):
    """lk_planes_sample for an array of hypotheses h: three distinct remainder positions below m each -> int64 [len(h), 3]."""
    with np.errstate(over="ignore"):
        ctr = (np.uint64(r) * np.uint64(LK_PLANES_MAX_HYP) + np.asarray(h, dtype=np.uint64)) * np.uint64(4) + np.uint64(int(seed) & _U64)
        i0 = planes_mulhi(planes_mix(ctr), m).astype(np.int64)
        i1 = planes_mulhi(planes_mix(ctr + np.uint64(1)), m - 1).astype(np.int64)
        i2 = planes_mulhi(planes_mix(ctr + np.uint64(2)), m - 2).astype(np.int64)
    i1 += i1 >= i0
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return np.stack([i0, i1, i2], axis=1)


def planes_status(cloud):
    p = np.asarray(cloud, dtype=np.float32).reshape(len(cloud), -1)[:, :3].astype(np.float64)
    fin = np.isfinite(p)
    return (0 if fin.all() else LK_PLANES_NONFINITE) | (LK_PLANES_RANGE if (np.abs(p[fin]) >= 2.0 ** 30).any() else 0)


def planes_hypotheses(p, idx, dist, axis=None, cos_max_angle=0.0, variant=None):
    """The hypotheses through the sampled records p[idx[:, 0 .. 2]] -> (a [H, 3], mvec [H, 3], t2q [H]); t2q is -1 where the hypothesis is skipped."""
    a, b, c = p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]]
    u, v = b - a, c - a
    mv = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    q = (mv[:, 0] * mv[:, 0] + mv[:, 1] * mv[:, 1]) + mv[:, 2] * mv[:, 2]
    ok = (q > 0.0) & np.isfinite(q)
    if axis is not None:
        ax = np.asarray(axis, dtype=np.float64)
        g = (mv[:, 0] * ax[0] + mv[:, 1] * ax[1]) + mv[:, 2] * ax[2]
        aa = 1.0 if variant == "axis_without_aa" else (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]
        ok &= ~(g * g < ((cos_max_angle * cos_max_angle) * q) * aa)
    if variant == "normalised":   # (what the definition avoids: a root and three divisions in front of every decision)
        with np.errstate(invalid="ignore", divide="ignore"):
            mv = np.where(ok[:, None], mv / np.sqrt(q)[:, None], mv)
        q = np.where(ok, 1.0, q)
    return a, mv, np.where(ok, (dist * dist) * q, -1.0)


def planes_inside(p, a, mv, t2q, variant=None, block=64, margin=None):
    """s * s <= t2q of every hypothesis against every record of p -> bool [H, m].  margin: a list whose entry 0 is lowered to the smallest
    |s * s - t2q| / t2q met among the hypotheses that are not skipped."""
    out = np.zeros((len(a), len(p)), dtype=bool)
    for b in range(0, len(a), block):
        e = p[None, :, :] - a[b:b + block, None, :]
        m = mv[b:b + block, None, :]
        s = (m[..., 0] * e[..., 0] + m[..., 1] * e[..., 1]) + m[..., 2] * e[..., 2]
        t = t2q[b:b + block, None]
        out[b:b + block] = (s * s < t) if variant == "strict" else (s * s <= t)
        if margin is not None and (t > 0.0).any() and len(p):
            margin[0] = min(margin[0], float((np.abs(s * s - t) / np.where(t > 0.0, t, 1.0))[(t > 0.0)[:, 0]].min()))
    return out


def planes_fit(pts, axis=None):
    """The reported coefficients of one plane from its inliers [n, 3] float64, sums in lk_planes_refit_kernel's order for a cloud that holds nothing
    else: centroid, covariance / n, eigh -> dict(normal, d, centroid, eig, rmse)."""
    n = len(pts)
    cen = np.array([sor_tree_sum(pts[:, k]) for k in range(3)]) / n
    dv = pts - cen
    c = {(i, j): sor_tree_sum(dv[:, i] * dv[:, j]) / n for i in range(3) for j in range(i, 3)}
    full = np.array([[c[min(i, j), max(i, j)] for j in range(3)] for i in range(3)])
    ev, vec = np.linalg.eigh(full)
    nrm = vec[:, 0]
    if axis is not None:
        flip = not (float(np.dot(nrm, np.asarray(axis, dtype=np.float64))) >= 0.0)
    else:
        flip = nrm[int(np.argmax(np.abs(nrm)))] < 0.0   # (argmax: the first among equals)
    nrm = -nrm if flip else nrm
    return dict(normal=nrm, d=-float(np.dot(nrm, cen)), centroid=cen, eig=ev, rmse=float(np.sqrt(max(ev[0], 0.0))))


def planes(cloud, dist, n_hyp, max_planes, min_inliers, axis=None, cos_max_angle=0.0, seed=0, flags=0, variant=None, cloud_index=0, trace=None):
    """The dominant planes of one cloud as lk_clouds_planes_dev defines them, by brute force: per round the sampler's three positions in the remainder,
    u x v, the score s * s <= dist^2 |u x v|^2 over the remainder, the largest score and the smallest h among equals; the winner's inliers become
    plane r and leave.  Returns a dict: label uint32 [m] (LK_PLANES_NONE: on no plane), keep bool [m], src_idx, planes (a list of dicts: normal, d,
    centroid, eig, rmse, n_inliers, hyp), and the record fields n_points, n_on_planes, n_rest, n_kept, n_planes, status.
    variant (test aid, one thing wrong each): PLANES_VARIANTS; cloud_index is read by "cloud_in_sampler" alone.  trace: a list that takes, per round,
    (the remainder's input indices, the sampled positions [H, 3], the scores [H], the winner, the smallest |s * s - t2q| / t2q of the round)."""
    m = len(cloud)
    pts = np.asarray(cloud, dtype=np.float32).reshape(m, -1)[:, :3].astype(np.float64) if m else np.zeros((0, 3))
    st = planes_status(cloud) if m else 0
    out = dict(label=np.full(m, LK_PLANES_NONE, dtype=np.uint32), keep=np.zeros(m, dtype=bool), src_idx=np.zeros(0, dtype=np.uint32), planes=[],
               n_points=m, n_on_planes=0, n_rest=0, n_kept=0, n_planes=0, status=st)
    if st:
        return out
    alive = np.ones(m, dtype=bool)
    hs = np.arange(n_hyp)
    sd = (int(seed) + (cloud_index << 40 if variant == "cloud_in_sampler" else 0)) & _U64
    for r in range(max_planes):
        rem = np.flatnonzero(alive)
        if len(rem) < max(3, min_inliers):
            break
        idx = planes_sample(sd, r, hs, len(rem))
        p = pts[rem]
        p_s = pts if variant == "input_indices" else p   # (the positions taken as indices of the INPUT: right in round 0 only)
        a, mv, t2q = planes_hypotheses(p_s, idx, dist, axis, cos_max_angle, variant)
        gap = [np.inf]
        inside = planes_inside(p, a, mv, t2q, variant, margin=gap if trace is not None else None)
        if variant == "samples_not_counted":
            for k in range(3):
                inside[hs, idx[:, k]] = False
        score = inside.sum(axis=1)
        w = int(len(score) - 1 - np.argmax(score[::-1])) if variant == "ties_last" else int(np.argmax(score))
        if trace is not None:
            trace.append((rem, idx, score.copy(), w, gap[0]))
        if score[w] < min_inliers:
            break
        members = rem[inside[w]]
        out["label"][members] = r
        alive[members] = False
        fit = planes_fit(pts[members], axis)
        fit.update(n_inliers=int(score[w]), hyp=w)
        out["planes"].append(fit)
    on = int((~alive).sum())
    keep = ~alive if flags & LK_PLANES_KEEP_PLANES else alive
    out.update(keep=keep, src_idx=np.flatnonzero(keep).astype(np.uint32), n_on_planes=on, n_rest=m - on, n_kept=int(keep.sum()), n_planes=len(out["planes"]))
    return out


def planes_clouds(clouds, dist, n_hyp, max_planes, min_inliers, axis=None, cos_max_angle=0.0, seed=0, flags=0, variant=None):
    """planes() of every cloud of one call -> a list of its dicts (variant "cloud_in_sampler": each with its index in the call)."""
    return [planes(c, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, variant, cloud_index=k) for k, c in enumerate(clouds)]
