"""The frozen table of relative-pose-error cases (lk_traj_rpe_dev, lk_runs_rpe_dev, tum.rpe): seeded, listed by name, small.

A case is a dict: est_t [n], est_pos [n, 3], est_rot [n, 3, 3], gt_t [m], gt_pos [m, 3], gt_rot [m, 3, 3] (float64, rotations row-major body -> world),
max_dt, and modes [q, 2]: the (delta, flags) pairs the case is evaluated under - flags 0 seconds, 1 LK_RPE_INDEX.  build() is the seeded generator;
the table the tests use (CASES) is its output as FROZEN in tests/golden/rpe_cases.npz, beside each case's figures, counts and term list evaluated at
50 digits from exactly those bits by the definition in include/legkilo_hip.h and rounded to float64.  tests/golden/make_rpe_cases.py writes the file;
tests/test_rpe_host.py checks that it regenerates to the bit and that build() still gives those inputs (to a few ulp).  The float64 numpy restatement
is legkilo_amd.tum.rpe.

TOLERANCE.  Translation figures (and term values): |x - x_50| <= C_T * 2^-53 * S, S = the largest absolute position coordinate among the poses of the
case's terms, at least 1.  Rotation figures: |x - x_50| <= C_R * 2^-53 * M^2, M = the largest absolute rotation entry among them, at least 1.  S and M
are per case and mode and stored in the file.  C_T and C_R are 16 x the worst ratio the numpy restatement reaches over this table, figures and term
values, every mode (the generator measures and prints them; the factor 16 is the project's margin for the same arithmetic in another order and another
libm, as in tests/atecases.py):
    NUMPY_RATIO_T = 3.37  (3.364 on "n257", the index step of 65)
    NUMPY_RATIO_R = 0.76  (0.754 on "rot_1e-9", the index step of 3)
    measured on the device (tests/test_rpe_gpu.py prints them): DEVICE_RATIO_T = 2.24, DEVICE_RATIO_R = 1.25.
tests/test_rpe_host.py re-measures the numpy ratios and fails beyond twice these (another BLAS rounds a 3 x 3 product differently; beyond a factor of
two the table or the restatement changed and the constants are stale).
WORST.  worst_trans / worst_rot are compared exactly wherever the 50-digit terms separate the largest from the runner-up by more than 4 tol; the
generator asserts that this holds for every case and mode with two terms or more, except
    TIES   built as exact ties ("identical": every term 0.0; "const_step": every step the same drift, in binary fractions) - worst_* must be the first
           term's index;
    RIGID  the pure rigid-transform cases: every term is zero but for the rounding of the transformed inputs, so no term can lead by 4 tol.  The
           generator asserts that all their terms lie below 4 tol, and the tests accept for worst_* any term within 4 tol of the largest - the
           comparison that is left when nothing separates them.  "noisy_rigid" is the rigid case WITH a separated worst term.
"""
import os

import numpy as np

from atecases import rot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpe_cases.npz")
KEYS = ("est_t", "est_pos", "est_rot", "gt_t", "gt_pos", "gt_rot")
FIGURES = ("trans_rmse", "trans_mean", "trans_max", "rot_rmse", "rot_mean", "rot_max")
NUMPY_RATIO_T = 3.37
NUMPY_RATIO_R = 0.76
DEVICE_RATIO_T = 2.24   # ("n129", the index step of 63)
DEVICE_RATIO_R = 1.25   # ("n64", 0.25 s)
C_T = 16.0 * NUMPY_RATIO_T
C_R = 16.0 * NUMPY_RATIO_R
ULP = 2.0 ** -53

SIZES = [0, 1, 2, 63, 64, 65, 129, 257]   # estimate sizes: wave-tile edges
TIES = ("identical", "const_step")
RIGID = ("rigid_yaw2_km", "rigid_tilt")


def rotz(a):
    c, s = np.cos(a), np.sin(a)
    z, o = np.zeros_like(c), np.ones_like(c)
    return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)


def planar(n, rng, rate=10.0):
    """A planar drive (yaw-only rotations, z = 0: the size cases stay small in the file) as ground truth, and as the estimate the same with 1 mm and
    1 mrad of noise and stamps jittered by up to 1 ms."""
    t = 100.0 + np.arange(n) / rate
    s = 0.05 * np.arange(n)
    gp = np.stack([6.0 * np.cos(s), 6.0 * np.sin(s), np.zeros(n)], axis=1)
    gr = rotz(s + np.pi / 2)
    ep = gp + 1e-3 * rng.normal(size=(n, 3))
    er = rotz(s + np.pi / 2 + 1e-3 * rng.normal(size=n))
    return t + 1e-3 * rng.uniform(-1, 1, size=n), ep, er, t, gp, gr


def spatial(n, rng, shift=(0.0, 0.0, 0.0), rate=10.0, noise=1e-3):
    """A rising spiral with rolling, pitching and yawing body as ground truth; the estimate = it with `noise` metres / radians of noise."""
    t = 100.0 + np.arange(n) / rate
    s = np.linspace(0.0, 1.7, n) if n > 1 else np.zeros(n)
    gp = np.stack([8.0 * np.cos(s), 8.0 * np.sin(s), 0.9 * s + 0.3 * np.sin(5 * s)], axis=1) + np.asarray(shift, dtype=np.float64)
    gr = np.array([rot([0, 0, 1], a + np.pi / 2) @ rot([1, 0, 0], 0.2 * np.sin(3 * a)) @ rot([0, 1, 0], 0.1 * np.cos(2 * a)) for a in s]).reshape(n, 3, 3)
    ep = gp + noise * rng.normal(size=(n, 3))
    er = np.array([Q @ rot(rng.normal(size=3), noise * rng.normal()) for Q in gr]).reshape(n, 3, 3)
    return t, ep, er, t.copy(), gp, gr


def moved(T_R, T_t, pos, rots):
    """One fixed rigid transform of a trajectory: R_i = T_R Q_i, p_i = T_R g_i + T_t."""
    return pos @ T_R.T + np.asarray(T_t, dtype=np.float64), np.array([T_R @ Q for Q in rots]).reshape(-1, 3, 3)


def case(est_t, est_pos, est_rot, gt_t, gt_pos, gt_rot, max_dt, modes):
    f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))   # noqa: E731
    return dict(est_t=f(est_t, (-1,)), est_pos=f(est_pos, (-1, 3)), est_rot=f(est_rot, (-1, 3, 3)), gt_t=f(gt_t, (-1,)), gt_pos=f(gt_pos, (-1, 3)),
                gt_rot=f(gt_rot, (-1, 3, 3)), max_dt=float(max_dt), modes=f(modes, (-1, 2)))


def build():
    rng = np.random.default_rng(20261021)
    up = lambda x: np.nextafter(x, np.inf)    # noqa: E731
    dn = lambda x: np.nextafter(x, -np.inf)   # noqa: E731
    cs = {}
    # ---- sizes.  Index steps 63 / 64 / 65: the far end's partner word belongs to another lane, or to the same lane one round on
    for n in SIZES:
        et, ep, er, gt, gp, gr = planar(max(n, 4), rng)
        modes = [(0.25, 0), (1, 1)]
        if n == 65:
            modes += [(64, 1)]
        if n == 129:
            modes += [(63, 1), (64, 1), (65, 1), (129, 1), (500, 1)]   # the last two: a step >= n_est
        if n == 257:
            modes = [(0.25, 0), (65, 1)]
        cs[f"n{n}"] = case(et[:n], ep[:n], er[:n], gt, gp, gr, 0.01, modes)   # n0: the empty estimate
    et, ep, er, gt, gp, gr = spatial(5, rng)
    cs["empty_gt"] = case(et, ep, er, gt[:0], gp[:0], gr[:0], 0.01, [(0.1, 0), (1, 1)])
    # ---- step search
    et, ep, er, gt, gp, gr = spatial(12, rng)
    t = 100.0 + 0.25 * np.arange(12)
    tt = t.copy()
    tt[4] = dn(tt[4])          # from i = 2 the target 101.0 lies one ulp ABOVE t[4]: k = 5; everywhere else t_i + delta == t_k exactly: k = i + 2
    cs["step_edges"] = case(tt, ep, er, t, gp, gr, 0.01, [(0.5, 0)])
    cs["step_past_end"] = case(t, ep, er, t, gp, gr, 0.01, [(1000.0, 0), (12, 1)])          # n_terms == 0 with n_pairs == 12
    cs["step_small"] = case(t, ep, er, t, gp, gr, 0.01, [(0.01, 0), (1, 1)])                # delta below the spacing: k = i + 1
    big = 1e8 + np.array([0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 4.0])                # ulp(1e8) = 1.5e-8 swallows delta = 1e-9: target == t_i,
    cs["dup_swallow"] = case(big, ep[:10], er[:10], 1e8 + np.arange(5.0), gp[:5], gr[:5], 0.01, [(1e-9, 0)])   # and k must still be i + 1
    # ---- pairing
    et, ep, er, gt, gp, gr = spatial(14, rng)
    off = et.copy()
    off[[5, 9, 10]] += 0.05    # samples 5, 9, 10 find no partner: steps 4 -> 5 (k unpaired), 5 -> 6 (i unpaired), 9 -> 10 (neither)
    cs["unpaired_ends"] = case(off, ep, er, gt, gp, gr, 0.01, [(0.1, 0), (1, 1), (0.2, 0)])
    te = 50.0 + np.arange(31) / 50.0
    tg = 50.0 + np.arange(7) / 10.0
    a = (tg - 50.0) * 1.5
    gp5 = np.stack([3 * np.cos(a), 3 * np.sin(a), 0.2 * a], axis=1)
    gr5 = np.array([rot([0, 0, 1], x) @ rot([1, 0, 0], 0.1 * x) for x in a])
    b = (te - 50.0) * 1.5
    ep5 = np.stack([3 * np.cos(b), 3 * np.sin(b), 0.2 * b], axis=1) + 1e-3 * rng.normal(size=(31, 3))
    er5 = np.array([rot([0, 0, 1], x) @ rot([1, 0, 0], 0.1 * x) @ rot(rng.normal(size=3), 1e-3 * rng.normal()) for x in b])
    cs["gt_fifth"] = case(te + 1e-5, ep5, er5, tg, gp5, gr5, 0.06, [(0.04, 0), (2, 1), (0.2, 0)])   # a fifth of the rate: steps with a == b
    et, ep, er, gt, gp, gr = spatial(8, rng)
    tg = np.arange(8.0)
    te = tg + 0.125
    te[2], te[5] = up(te[2]), up(te[5])   # |dt| == max_dt pairs, one ulp above does not: at the far end of step 1 -> 2, at the near end of 2 -> 3, ...
    tm = tg - 0.125
    tm[3], tm[6] = dn(tm[3]), dn(tm[6])
    cs["dt_edges"] = case(te, ep, er, tg, gp, gr, 0.125, [(1.0, 0), (1, 1)])
    cs["dt_edges_before"] = case(tm, ep, er, tg, gp, gr, 0.125, [(1.0, 0), (1, 1)])
    cs["midway"] = case(tg[:7] + 0.5, ep[:7], er[:7], tg, gp, gr, 0.5, [(1.0, 0), (1, 1)])   # midway between two ground-truth stamps: the earlier one
    # ---- geometry
    et, ep, er, gt, gp, gr = spatial(20, rng)
    cs["identical"] = case(gt, gp, gr, gt, gp, gr, 0.01, [(0.3, 0), (1, 1), (7, 1)])          # exactly 0.0
    T1, t1 = rot([0, 0, 1], 2.0), [3600.0, -2500.0, 40.0]
    mp, mr = moved(T1, t1, gp, gr)
    cs["rigid_yaw2_km"] = case(gt, mp, mr, gt, gp, gr, 0.01, [(0.3, 0), (1, 1)])
    T2, t2 = rot([0.3, -0.5, 0.8], 0.7), [0.5, -0.25, 0.125]
    mp, mr = moved(T2, t2, gp, gr)
    cs["rigid_tilt"] = case(gt, mp, mr, gt, gp, gr, 0.01, [(0.3, 0), (1, 1)])
    for name, shift in (("noisy_origin", (0, 0, 0)), ("noisy_3p6km", (3600.0, -3600.0, 12.0)), ("noisy_600km", (6e5, 6e5, -300.0))):
        et, ep, er, gt, gp, gr = spatial(24, rng, shift=shift)
        cs[name] = case(et, ep, er, gt, gp, gr, 0.01, [(0.3, 0), (1, 1)])
    c0 = cs["noisy_origin"]
    mp, mr = moved(T1, t1, c0["est_pos"], c0["est_rot"])
    cs["noisy_rigid"] = case(c0["est_t"], mp, mr, c0["gt_t"], c0["gt_pos"], c0["gt_rot"], 0.01, [(0.3, 0), (1, 1)])   # noisy_origin's figures
    # relative rotations of 1e-9 rad, 90, 179.9 and exactly 180 degrees about an axis, one per step; the ground truth does not turn
    ax = np.array([0.3, -0.5, 0.8])
    Rs = [np.eye(3)]
    for R in (rot(ax, 1e-9), rot(ax, np.pi / 2), rot([1, 2, -1], np.deg2rad(179.9)), np.diag([1.0, -1.0, -1.0]), rot(ax, 0.01)):
        Rs.append(Rs[-1] @ R)
    t6 = 10.0 + np.arange(6.0)
    p6 = np.outer(np.arange(6.0), [0.5, 0.25, -0.125])
    cs["rot_angles"] = case(t6, p6, Rs, t6, p6, [np.eye(3)] * 6, 0.01, [(1.0, 0), (1, 1)])
    cs["rot_180_exact"] = case(t6[:2], p6[:2], [np.eye(3), np.diag([1.0, -1.0, -1.0])], t6[:2], p6[:2], [np.eye(3)] * 2, 0.01, [(1, 1)])
    n = 16
    t16 = 20.0 + np.arange(n) / 10.0
    yaw = 0.1 * np.arange(n)
    p16 = np.outer(np.arange(n), [0.5, 0.25, -0.125])
    cs["rot_1e-9"] = case(t16, p16 + 1e-3 * rng.normal(size=(n, 3)), rotz(yaw + 1e-9 * np.arange(n) ** 2), t16, p16, rotz(yaw), 0.01, [(0.1, 0), (1, 1), (3, 1)])
    et, ep, er, gt, gp, gr = spatial(20, rng)
    cs["gt_scaled"] = case(et, ep, er, gt, gp, gr * (1.0 + 1e-6), 0.01, [(0.3, 0), (1, 1)])   # not orthonormal: the formula defines the expectation
    spot = np.tile([2.0, -1.0, 0.5], (20, 1))   # the body turns on the spot; the estimate's position wanders by a millimetre about it
    cs["pure_rotation"] = case(et, spot + 1e-3 * rng.normal(size=(20, 3)), er, gt, spot, gr, 0.01, [(0.3, 0), (1, 1)])
    noisy_eye = np.array([rot(rng.normal(size=3), 1e-3 * rng.normal()) for _ in range(20)])
    cs["pure_translation"] = case(et, ep, noisy_eye, gt, gp, [np.eye(3)] * 20, 0.01, [(0.3, 0), (1, 1)])
    g8 = np.outer(np.arange(8.0), [0.5, 0.25, -0.125])
    t8 = 20.0 + 0.25 * np.arange(8)   # (binary fractions: t_i + 0.25 == t_(i+1) exactly)
    cs["const_step"] = case(t8, g8 + np.outer(np.arange(8.0), [2.0 ** -7, 0, 0]), [np.eye(3)] * 8, t8, g8, [np.eye(3)] * 8, 0.01, [(0.25, 0), (1, 1), (2, 1)])
    # ---- non-finite values
    et, ep, er, gt, gp, gr = spatial(20, rng)
    bad = ep.copy()
    bad[7, 1] = np.nan
    cs["nan_pos_term"] = case(et, bad, er, gt, gp, gr, 0.01, [(0.3, 0), (1, 1)])
    badr = gr.copy()
    badr[7, 1, 2] = np.nan
    cs["nan_rot_term"] = case(et, ep, er, gt, gp, badr, 0.01, [(0.3, 0), (1, 1)])
    badi = er.copy()
    badi[7, 0, 0] = np.inf
    off = et.copy()
    off[7] += 0.05
    both = bad.copy()
    cs["nan_unpaired"] = case(off, both, badi, gt, gp, gr, 0.01, [(0.3, 0), (1, 1)])          # sample 7 has no partner: its pose is never read
    cs["nan_no_term"] = case(et, bad, badi, gt, gp, gr, 0.01, [(1.45, 0), (15, 1)])           # steps 0..4 -> 15..19: samples 5 .. 14 are in no term
    return cs


def pack(d):
    """{key: float64 or int64 array} -> the four arrays of the file: hundreds of small arrays as members of an .npz cost more than their content, so
    the values lie in one float64 and one int64 array, with the keys, their shapes (padded to three dimensions with -1) and their offsets beside."""
    keys = list(d)
    blobs, index = {"f": [], "i": []}, []
    fill = {"f": 0, "i": 0}
    for k in keys:
        v = np.asarray(d[k])
        kind = {"float64": "f", "int64": "i"}[str(v.dtype)]
        index.append([kind == "i", fill[kind]] + list(v.shape) + [-1] * (3 - v.ndim))
        blobs[kind].append(v.ravel())
        fill[kind] += v.size
    return dict(keys=np.array(keys), index=np.array(index, dtype=np.int64).reshape(-1, 5), f64=np.concatenate(blobs["f"] + [np.zeros(0)]),
                i64=np.concatenate(blobs["i"] + [np.zeros(0, dtype=np.int64)]))


def unpack(z):
    out = {}
    for k, (is_int, off, *shape) in zip(z["keys"], z["index"]):
        shape = [int(x) for x in shape if x >= 0]
        n = int(np.prod(shape)) if shape else 1
        out[str(k)] = (z["i64"] if is_int else z["f64"])[int(off):int(off) + n].reshape(shape).copy()
    return out


def golden():
    """Everything in tests/golden/rpe_cases.npz as {key: array}: `name/in/<field>` and `name/m<q>/<field>`."""
    return unpack(np.load(GOLDEN))


def load():
    """The frozen inputs of tests/golden/rpe_cases.npz, in the table's order."""
    z = golden()
    names = list(dict.fromkeys(k.split("/")[0] for k in z))
    return {n: dict({k: z[f"{n}/in/{k}"] for k in KEYS}, max_dt=float(z[f"{n}/in/max_dt"][0]), modes=z[f"{n}/in/modes"]) for n in names}


CASES = load() if os.path.exists(GOLDEN) else build()
NAMES = list(CASES)


def modes(c):
    """[(q, delta, flags)] of a case."""
    return [(q, float(d), int(f)) for q, (d, f) in enumerate(c["modes"])]


def tol_t(S):
    return C_T * ULP * max(1.0, S)


def tol_r(M):
    return C_R * ULP * max(1.0, M) ** 2


def expected(z, name, q):
    """The 50-digit record of case `name` under its mode q, from golden()."""
    k = f"{name}/m{q}/"
    fig, cnt = z[k + "figures"], z[k + "counts"]
    return dict(dict(zip(FIGURES, fig)), n_terms=int(cnt[0]), n_pairs=int(cnt[1]), status=int(cnt[2]), worst_trans=int(cnt[3]), worst_rot=int(cnt[4]),
                terms=z[k + "terms"], e_t=z[k + "e_t"], e_r=z[k + "e_r"], margins=z[k + "margins"], S=float(z[k + "scale"][0]), M=float(z[k + "scale"][1]))


def check(name, got, want):
    """A record (anything indexable by the field names) against the 50-digit one: counts and status exactly, figures within the tolerance (NaN meets
    NaN), worst_* by the rule above.  Returns the ratios (translation, rotation) the figures reach."""
    for f in ("n_terms", "n_pairs", "status"):
        assert int(got[f]) == want[f], (name, f, int(got[f]), want[f])
    ratios = [0.0, 0.0]
    for h, unit in enumerate((ULP * want["S"], ULP * want["M"] ** 2)):
        for f in FIGURES[3 * h:3 * h + 3]:
            if np.isnan(want[f]):
                assert np.isnan(got[f]), (name, f, got[f])
            else:
                assert np.isfinite(got[f]), (name, f, got[f])
                ratios[h] = max(ratios[h], abs(float(got[f]) - float(want[f])) / unit)
    assert ratios[0] <= C_T and ratios[1] <= C_R, (name, ratios, (C_T, C_R))
    if want["n_terms"] == 0 or want["status"]:
        assert (int(got["worst_trans"]), int(got["worst_rot"])) == (0, 0), name
        return ratios
    first = want["terms"][:, 0]
    for f, e, tol, margin in (("worst_trans", want["e_t"], tol_t(want["S"]), want["margins"][0]), ("worst_rot", want["e_r"], tol_r(want["M"]), want["margins"][1])):
        w = int(got[f])
        if name in TIES:
            assert w == int(first[0]), (name, f, w)
        elif margin > 4 * tol:
            assert w == want[f], (name, f, w, want[f])
        else:   # nothing separates the largest terms (RIGID, or a single term): any term within 4 tol of the largest
            assert w in first and e[list(first).index(w)] >= e.max() - 4 * tol, (name, f, w)
    return ratios
