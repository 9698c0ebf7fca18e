"""The float64 numpy restatement of lk_traj_rpe_dev on a case of tests/rpecases.py - legkilo_amd.tum.rpe itself - and deliberately WRONG restatements
beside it (tests/test_rpe_host.py shows that each one fails on a named case of the table):
    "from0"    the step searched from index 0 instead of from i + 1;
    "strict"   the step's far end needs t_est[k] > target instead of >=;
    "later"    the later ground-truth sample wins on equal distance;
    "world"    world-frame displacement differences, |(p_k - p_i) - (g_b - g_a)|;
    "acos"     e_r = arccos(c) instead of arctan2(s, c);
    "reortho"  the matrices re-orthonormalised (nearest rotation) before use."""
import numpy as np

from legkilo_amd import tum

NONFINITE = 1
VARIANTS = ("from0", "strict", "later", "world", "acos", "reortho")


def args(c, delta, flags):
    return (c["est_t"], c["est_pos"], c["est_rot"], c["gt_t"], c["gt_pos"], c["gt_rot"], c["max_dt"], delta), dict(by_index=bool(flags))


def nearest_rotation(R):
    U, _, Vt = np.linalg.svd(R)
    return U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt


def rpe(c, delta, flags, variant=None):
    """One case under one mode -> tum.rpe's dict."""
    a, kw = args(c, delta, flags)
    if variant is None:
        return tum.rpe(*a, **kw)
    assert variant in VARIANTS
    et, gt_t, n = c["est_t"], c["gt_t"], len(c["est_t"])
    part = tum.rpe_partners(et, gt_t, c["max_dt"])
    if variant == "later" and len(gt_t):
        for i, te in enumerate(et):
            d = np.abs(te - gt_t)
            j = int(np.flatnonzero(d == d.min())[-1])
            part[i] = j if d[j] <= c["max_dt"] else -1
    step = tum.rpe_steps(et, delta, bool(flags))
    if not flags and variant in ("from0", "strict"):
        for i in range(n):
            target = et[i] + delta
            ks = [k for k in range(0 if variant == "from0" else i + 1, n) if (et[k] > target if variant == "strict" else et[k] >= target)]
            step[i] = ks[0] if ks else -1
    terms = np.array([(i, k, part[i], part[k]) for i, k in enumerate(step) if k >= 0 and part[i] >= 0 and part[k] >= 0], dtype=np.int64).reshape(-1, 4)
    res = tum.rpe(*a, **kw)
    res = dict(res, terms=terms, n_terms=len(terms), n_pairs=int((part >= 0).sum()))
    if len(terms) == 0 or res["status"]:
        return res
    fix = nearest_rotation if variant == "reortho" else (lambda R: R)
    e_t, e_r = [], []
    for i, k, a_, b in terms:
        Ri, Rk, Qa, Qb = fix(c["est_rot"][i]), fix(c["est_rot"][k]), fix(c["gt_rot"][a_]), fix(c["gt_rot"][b])
        t, s, cc = tum.rpe_term(Ri, c["est_pos"][i], Rk, c["est_pos"][k], Qa, c["gt_pos"][a_], Qb, c["gt_pos"][b])
        if variant == "world":
            d = (c["est_pos"][k] - c["est_pos"][i]) - (c["gt_pos"][b] - c["gt_pos"][a_])
            t = float(np.sqrt((d * d).sum()))
        e_t.append(t)
        e_r.append(float(np.arccos(np.clip(cc, -1.0, 1.0))) if variant == "acos" else float(np.arctan2(s, cc)))
    e_t, e_r = np.array(e_t), np.array(e_r)
    res.update(trans_rmse=float(np.sqrt((e_t * e_t).mean())), trans_mean=float(e_t.mean()), trans_max=float(e_t.max()),
               rot_rmse=float(np.sqrt((e_r * e_r).mean())), rot_mean=float(e_r.mean()), rot_max=float(e_r.max()),
               worst_trans=int(terms[int(np.argmax(e_t)), 0]), worst_rot=int(terms[int(np.argmax(e_r)), 0]), e_t=e_t, e_r=e_r)
    return res
