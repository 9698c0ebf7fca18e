"""TUM trajectory I/O and ATE — the on-disk format the parity metric of the north star
("trajectory ATE delta < 1 mm") is defined on.

write_tum() follows TrajectorySaver::write (legkilo/src/common/trajectory_saver.hpp:43-50):
    `timestamp tx ty tz qx qy qz qw`, fixed notation, 9 decimals, rotation = body -> world,
    quaternion from the rotation matrix the way Eigen::Quaterniond(Matrix3d) does (Shepperd's branches).
ate() is the usual absolute trajectory error: associate by time stamp, optionally align with the
closed-form rigid (Horn / Umeyama without scale) transform, RMSE of the position differences.
Host-side utility; no device code is involved.
"""
import numpy as np


def rot_to_quat(R):
    """Eigen::Quaterniond(Matrix3d): returns (x, y, z, w)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        x, y, z = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = [0.0, 0.0, 0.0]
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
        x, y, z = q
    return x, y, z, w


def write_tum(path, stamps, rots, poss):
    with open(path, "w") as f:
        for t, R, p in zip(stamps, rots, poss):
            x, y, z, w = rot_to_quat(R)
            f.write("%.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n" % (t, p[0], p[1], p[2], x, y, z, w))


def read_tum(path):
    a = np.loadtxt(path, ndmin=2)
    return a[:, 0], a[:, 1:4], a[:, 4:8]


def associate(ta, tb, max_dt=0.01):
    """Greedy nearest-stamp association (both sorted): index pairs with |dt| <= max_dt."""
    ia, ib, out = 0, 0, []
    while ia < len(ta) and ib < len(tb):
        d = ta[ia] - tb[ib]
        if abs(d) <= max_dt:
            out.append((ia, ib))
            ia += 1
            ib += 1
        elif d < 0:
            ia += 1
        else:
            ib += 1
    return np.array(out, dtype=int).reshape(-1, 2)


def ate(pa, pb, align=False):
    """RMSE of position differences; align=True removes the best rigid transform b -> a first."""
    pa, pb = np.asarray(pa, float), np.asarray(pb, float)
    if align:
        ca, cb = pa.mean(0), pb.mean(0)
        H = (pb - cb).T @ (pa - ca)
        U, _, Vt = np.linalg.svd(H)
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
        R = Vt.T @ D @ U.T
        pb = (pb - cb) @ R.T + ca
    d = pa - pb
    return float(np.sqrt((d * d).sum(1).mean()))


def quat_to_rot(q_xyzw):
    """Quaternions (x, y, z, w) [..., 4], as read_tum hands them out, -> row-major rotation matrices [..., 3, 3]; the quaternion is normalised
    first (a TUM file carries 9 decimals).  The step between a ground-truth file and the rotation tables of lk_traj_rpe_dev."""
    q = np.asarray(q_xyzw, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = (w * w + x * x) - (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2.0 * (x * y + w * z), (w * w + y * y) - (x * x + z * z), 2.0 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2.0 * (x * z - w * y), 2.0 * (y * z + w * x), (w * w + z * z) - (x * x + y * y)
    return R


def rpe_partners(est_t, gt_t, max_dt):
    """int64 [n]: per estimate sample the ground-truth sample that minimises fabs(est_t[i] - gt_t[j]), the earliest on equal distance, or -1 when
    that distance exceeds max_dt (or there is no ground truth) - the association of lk_traj_ate_dev / lk_traj_rpe_dev."""
    est_t, gt_t = np.asarray(est_t, np.float64).reshape(-1), np.asarray(gt_t, np.float64).reshape(-1)
    out = np.full(len(est_t), -1, dtype=np.int64)
    if len(gt_t):
        for i, te in enumerate(est_t):
            d = np.abs(te - gt_t)
            j = int(np.argmin(d))
            if d[j] <= max_dt:
                out[i] = j
    return out


def rpe_steps(est_t, delta, by_index=False):
    """int64 [n]: k(i), the far end of the step that starts at estimate sample i, or -1 - the first k > i with est_t[k] >= est_t[i] + delta
    (by_index: i + int(delta))."""
    est_t = np.asarray(est_t, np.float64).reshape(-1)
    n = len(est_t)
    out = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        k = i + int(delta) if by_index else i + 1 + int(np.searchsorted(est_t[i + 1:], est_t[i] + delta, side="left"))
        if k < n:
            out[i] = k
    return out


def rpe_term(Ri, pi, Rk, pk, Qa, ga, Qb, gb):
    """One step: (e_t, s, c) of the header's formula - translation error, sine and cosine of the rotation error; e_r = arctan2(s, c)."""
    dRe, dpe = Ri.T @ Rk, Ri.T @ (pk - pi)
    dRg, dpg = Qa.T @ Qb, Qa.T @ (gb - ga)
    d = dpe - dpg
    E = dRg.T @ dRe
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.sqrt((d * d).sum())), 0.5 * float(np.sqrt((v * v).sum())), 0.5 * (E[0, 0] + E[1, 1] + E[2, 2] - 1.0)


def rpe(est_t, est_pos, est_rot, gt_t, gt_pos, gt_rot, max_dt, delta, by_index=False):
    """Relative pose error as lk_traj_rpe_dev defines it (include/legkilo_hip.h), in float64 numpy: stamps [n], positions [n, 3], rotations
    [n, 3, 3] (body -> world) of the estimate and of the ground truth.  Sample i and the first later sample k at least `delta` seconds on (by_index:
    `delta` samples on) make a term when both have a ground-truth partner within max_dt (nearest stamp, the earliest on ties); the term compares
    the estimate's motion i -> k with the partners' motion, both in the first pose's frame.
    Returns a dict: trans_rmse / trans_mean / trans_max (metres), rot_rmse / rot_mean / rot_max (radians), n_terms, n_pairs, worst_trans / worst_rot
    (the i of the largest term, first on ties), status (1: a pose of a term is not finite - the figures are then NaN), and the term list itself:
    terms int64 [n_terms, 4] = (i, k, a, b), e_t / e_r float64 [n_terms]."""
    est_pos, gt_pos = np.asarray(est_pos, np.float64).reshape(-1, 3), np.asarray(gt_pos, np.float64).reshape(-1, 3)
    est_rot, gt_rot = np.asarray(est_rot, np.float64).reshape(-1, 3, 3), np.asarray(gt_rot, np.float64).reshape(-1, 3, 3)
    part, step = rpe_partners(est_t, gt_t, max_dt), rpe_steps(est_t, delta, by_index)
    terms = np.array([(i, k, part[i], part[k]) for i, k in enumerate(step) if k >= 0 and part[i] >= 0 and part[k] >= 0], dtype=np.int64).reshape(-1, 4)
    nan = float("nan")
    res = dict(trans_rmse=nan, trans_mean=nan, trans_max=nan, rot_rmse=nan, rot_mean=nan, rot_max=nan, n_terms=len(terms), n_pairs=int((part >= 0).sum()),
               worst_trans=0, worst_rot=0, status=0, terms=terms, e_t=np.zeros(0), e_r=np.zeros(0))
    if len(terms) == 0:
        return res
    i, k, a, b = terms.T
    if not all(np.isfinite(v).all() for v in (est_pos[i], est_pos[k], est_rot[i], est_rot[k], gt_pos[a], gt_pos[b], gt_rot[a], gt_rot[b])):
        res["status"] = 1
        return res
    v = np.array([rpe_term(est_rot[i_], est_pos[i_], est_rot[k_], est_pos[k_], gt_rot[a_], gt_pos[a_], gt_rot[b_], gt_pos[b_]) for i_, k_, a_, b_ in terms])
    e_t, e_r = v[:, 0], np.arctan2(v[:, 1], v[:, 2])
    res.update(trans_rmse=float(np.sqrt((e_t * e_t).mean())), trans_mean=float(e_t.mean()), trans_max=float(e_t.max()),
               rot_rmse=float(np.sqrt((e_r * e_r).mean())), rot_mean=float(e_r.mean()), rot_max=float(e_r.max()),
               worst_trans=int(i[int(np.argmax(e_t))]), worst_rot=int(i[int(np.argmax(e_r))]), e_t=e_t, e_r=e_r)
    return res


def ate_files(path_a, path_b, align=False, max_dt=0.01):
    ta, pa, _ = read_tum(path_a)
    tb, pb, _ = read_tum(path_b)
    m = associate(ta, tb, max_dt)
    if len(m) == 0:
        raise ValueError("no associated stamps")
    return ate(pa[m[:, 0]], pb[m[:, 1]], align), len(m)
