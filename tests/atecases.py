"""The frozen table of trajectory-error cases (lk_traj_ate_dev, lk_runs_ate_dev): seeded, listed by name, small.

A case is a dict: est_t [n], est_pos [n, 3], gt_t [m], gt_pos [m, 3] (float64), max_dt.  Every case is evaluated with and without LK_ATE_ALIGN.
build() is the seeded generator; the table the tests use (CASES) is its output as FROZEN in tests/golden/ate_cases.npz, beside each case's figures
evaluated at 50 digits and rounded to float64 - so the expected values belong to exactly the bits the tests feed, whatever a platform's cos or
normal() rounds to.  tests/golden/make_ate_cases.py writes the file; tests/test_ate_host.py checks that the figures regenerate to the bit from the
frozen inputs and that build() still gives those inputs (to a few ulp).  tests/ate_ref.py is the float64 numpy restatement.

TOLERANCE.  |x_dev - x_50| <= C * 2^-53 * S for rmse, mean and max, S = the case's largest absolute finite coordinate (scale()).
C = 16 * max(1, worst ratio |x_numpy - x_50| / (2^-53 * S) the float64 numpy restatement reaches over this table): the factor 16 covers another
summation order and another solver (tests/test_filter_solvers.py reasons the same way).  Measured on this table, both flags, all three figures:
    NUMPY_RATIO = 4.99  (4.989 on "arc_600km" aligned, then 4.59 "n257" aligned, 3.60 "rate_500_100_wide" aligned, 3.16 "midway" aligned; without
                         alignment no case exceeds 0.9; figure by figure the worst is "max", a single e_i that nothing averages)
so C = 16 * 4.99 = 79.84.  tests/test_ate_host.py re-measures and prints the ratio, and fails if it exceeds twice NUMPY_RATIO (another LAPACK build
rounds the SVD differently; beyond a factor of two the table or the restatement changed and C is stale).
The worst pair's index is compared exactly where the 50-digit values separate it from the runner-up by more than 2 tol(case) (each e_i may be off by
tol): elsewhere two pairs tie within what either side can resolve.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ate_cases.npz")
KEYS = ("est_t", "est_pos", "gt_t", "gt_pos")
NUMPY_RATIO = 4.99
C = 16.0 * max(1.0, NUMPY_RATIO)
ULP = 2.0 ** -53

SIZES = [0, 1, 2, 3, 63, 64, 65, 129, 257]   # paired sizes: wave-tile edges


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def arc(n, rng, noise=1e-8, shift=(0.0, 0.0, 0.0), rate=10.0):
    """A 3-D arc (a rising spiral of ~8 m radius) as ground truth and the same under a rigid motion with `noise` metres of noise as the estimate."""
    t = 100.0 + np.arange(n) / rate
    s = np.linspace(0.0, 1.7, n) if n > 1 else np.zeros(n)
    gt = np.stack([8.0 * np.cos(s), 8.0 * np.sin(s), 0.9 * s + 0.3 * np.sin(5 * s)], axis=1) + np.asarray(shift, dtype=np.float64)
    R = rot([0.3, -0.5, 0.8], 0.4)
    est = (gt - gt.mean(0)) @ R.T + gt.mean(0) + np.array([0.5, -0.25, 0.125]) + noise * rng.normal(size=(n, 3))
    return t, gt, est


def case(est_t, est_pos, gt_t, gt_pos, max_dt):
    f = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))   # noqa: E731
    return dict(est_t=f(est_t, (-1,)), est_pos=f(est_pos, (-1, 3)), gt_t=f(gt_t, (-1,)), gt_pos=f(gt_pos, (-1, 3)), max_dt=float(max_dt))


def build():
    rng = np.random.default_rng(20261020)
    cs = {}
    # ---- sizes: n paired samples; n0 has three estimate samples, all out of reach
    for n in SIZES:
        if n == 0:
            t, gt, est = arc(3, rng)
            cs["n0"] = case(t + 0.05, est, t, gt, 0.01)
        else:
            t, gt, est = arc(n, rng)
            cs[f"n{n}"] = case(t + 1e-3 * rng.uniform(-1, 1, size=n), est, t, gt, 0.01)
    t, gt, est = arc(5, rng)
    cs["empty_est"] = case(t[:0], est[:0], t, gt, 0.01)
    cs["empty_gt"] = case(t, est, t[:0], gt[:0], 0.01)
    cs["single_gt"] = case(t, est, t[2:3], gt[2:3], 0.25)   # samples 0 .. 4 lie 0.2, 0.1, 0, 0.1, 0.2 s away: all five pair with the one sample
    # ---- stamps
    gt_t = np.arange(6, dtype=np.float64)
    gp = rng.normal(size=(6, 3))
    ep = rng.normal(size=(5, 3))
    cs["midway"] = case(gt_t[:5] + 0.5, ep, gt_t, gp, 0.5)           # exactly midway between two samples: the earlier one wins
    up = lambda x: np.nextafter(x, np.inf)                             # noqa: E731
    dn = lambda x: np.nextafter(x, -np.inf)                            # noqa: E731
    et = np.array([1.0 + 0.125, up(2.0 + 0.125), 3.0 - 0.125, dn(4.0 - 0.125), 5.0 + 0.0625])
    cs["dt_exact"] = case(et, ep, gt_t * 1.0, gp, 0.125)            # |dt| == max_dt pairs (samples 0, 2), one ulp above does not (1, 3)
    t, gt, est = arc(9, rng)
    et = np.r_[t[0] - 1.0, t[0] - 0.004, t[1:8] + 0.002, t[8] + 0.004, t[8] + 1.0]
    cs["outside"] = case(et, np.r_[est[:1], est, est[-1:]], t, gt, 0.01)   # before the first and behind the last ground-truth stamp, in and out of reach
    t, gt, est = arc(8, rng)
    tg = t.copy()
    tg[3] = tg[2]
    tg[6] = tg[5] = tg[4]
    cs["dup_gt"] = case(np.r_[t[:4] + 0.003, t[4], t[5:7] + 0.003, t[7]], est, tg, gt, 0.2)   # equal ground-truth stamps, met from behind, from the front and exactly: the earliest of them
    m = 26
    tg = 50.0 + np.arange(m) / 100.0
    te = 50.0 + np.arange(5 * (m - 1) + 1) / 500.0 + 1e-5
    s = (tg - 50.0) * 4
    gt = np.stack([3 * np.cos(s), 3 * np.sin(s), 0.2 * s], axis=1)
    se = (te - 50.0) * 4
    est = np.stack([3 * np.cos(se), 3 * np.sin(se), 0.2 * se], axis=1) + 1e-3 * rng.normal(size=(len(te), 3))
    cs["rate_500_100"] = case(te, est, tg, gt, 1e-3)                # 500 Hz against 100 Hz: every fifth sample pairs
    cs["rate_500_100_wide"] = case(te, est, tg, gt, 5e-3)           # ... every sample does, a ground-truth sample serves five: NOT tum.associate's pairs
    # ---- geometry
    for name, shift in (("arc_origin", (0, 0, 0)), ("arc_3p6km", (3600.0, -3600.0, 12.0)), ("arc_600km", (6e5, 6e5, -300.0))):
        t, gt, est = arc(100, rng, shift=shift)
        cs[name] = case(t, est, t, gt, 0.01)
    t, gt, est = arc(40, rng)
    gt[:, 2] = 0.0
    R = rot([0.1, 0.2, 1.0], 0.7)
    cs["planar"] = case(t, gt @ R.T + 1e-8 * rng.normal(size=gt.shape) + 2.0, t, gt, 0.01)
    t, gt, est = arc(40, rng)
    cs["mirrored"] = case(t, gt * np.array([1.0, 1.0, -1.0]) + 1e-8 * rng.normal(size=gt.shape), t, gt, 0.01)   # the best orthogonal map is a reflection
    t = 10.0 + np.arange(12) / 10.0
    line = np.outer(np.linspace(-3, 4, 12), [0.6, -0.3, 0.74]) + 1.5
    cs["collinear"] = case(t, (line - 1.5) @ rot([1, 1, 0], 1.1).T + 1e-8 * rng.normal(size=line.shape), t, line, 0.01)
    cs["coincident2"] = case([1.0, 2.0], [[0.5, 0.25, -1.0], [0.5, 0.25, -1.0]], [1.0, 2.0], [[2.0, 3.0, 4.0], [2.0, 3.0, 4.0]], 0.01)
    t, gt, est = arc(70, rng)
    cs["identical"] = case(t, gt, t, gt, 0.01)                       # without align: exactly 0.0
    t, gt, est = arc(20, rng)
    bad = est.copy()
    bad[7, 1] = np.nan
    cs["nan_paired"] = case(t, bad, t, gt, 0.01)
    et = t.copy()
    et[7] += 0.05
    cs["nan_unpaired"] = case(et, bad, t, gt, 0.01)                  # the NaN sits in a sample that has no partner: never read
    return cs


def load():
    """The frozen inputs of tests/golden/ate_cases.npz, in the table's order."""
    z = np.load(GOLDEN)
    return {str(n): dict({k: z[f"{n}/in/{k}"] for k in KEYS}, max_dt=float(z[f"{n}/in/max_dt"][0])) for n in z["names"]}


CASES = load() if os.path.exists(GOLDEN) else build()
NAMES = list(CASES)
FLAGS = (0, 1)   # without / with LK_ATE_ALIGN


def scale(c):
    v = np.concatenate([c["est_pos"].ravel(), c["gt_pos"].ravel()])
    v = np.abs(v[np.isfinite(v)])
    return float(v.max()) if v.size else 1.0


def tol(c):
    return C * ULP * scale(c)
