"""Systems that make the filter's Gauss-Jordan solvers pivot: the frozen case table, 50-digit references, numpy restatements.

The Kalman correction exists in five hand-written copies of one solver (dev_solve, the one-column-per-lane forms of wave_update_core /
wave_imu_update_core / wave_kin_update_core, the oracle's 6 x 6 information form).  The parity tests feed them nearly diagonal priors and
isotropic rows: no copy ever swaps a row there.  The cases here do - correlated priors whose sigmas span decades, rows [p x n, n] with
nearly parallel normals - and every property a case is listed for (its swap list under exact arithmetic, the 1.5 margin of every pivot
decision, the caps on kappa_inf(S)) is asserted by assert_case, which every test calls before it looks at a result.

  POINT_CASES   x36, P (30 x 30), h6 (N x 6), z, R        S = I + A P66 (6 x 6, NOT symmetric), A = sum h h^T / R
  IMU_CASES     x36, P, z6, R6                            S = H P H^T + R, H = 1 on columns 9..14 and 18..23
  DENSE_CASES   x36, P, a kinematic + IMU record          S = H P H^T + R, rows of msgcases.kin_rows (KILO.cc:267-309), M = 6 + 3 contacts

Cases were found by a seeded search (parameters below are its frozen outcome) and are rebuilt from their seeds; tests/golden/
solver_cases.npz holds the inputs and the 50-digit results rounded to float64, test_filter_solvers.py regenerates it to the bit.

The criterion (EPS = 2^-53, kappa = kappa_inf of the 50-digit S, all maxima over entries):

  covariance   max |P_test - P_50|  <= C * EPS * kappa * max |P_prior|
  state step   max |dx_test - dx_50| <= C * EPS * kappa * max |dx_50|
  asymmetry    max |P' - P'^T|       <= twice the covariance bound

C is 16 times the largest err / (EPS * kappa * scale) the float64 restatements below reach on the table (RATIO_MEASURED): the 16 covers
FMA contraction and another summation order - rounding-level effects - while a pivoting mistake is off by a factor of order one.
"""
import functools
import os

import numpy as np
from mpmath import mp, mpf

import msgcases as mc
from legkilo_amd import synth

mp.dps = 50
EPS = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_cases.npz")
KAPPA_CAP, KAPPA_LOW = 1e6, 1e3
MARGIN = 1.5


# ----------------------------------------------------------------------------- building blocks of the cases
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rodrigues(v):
    n = np.linalg.norm(v)
    K = skew(v / n)
    return np.eye(3) + np.sin(n) * K + (1 - np.cos(n)) * K @ K


def block_prior(rng, spec, nfac, floor):
    """SPD prior: sigmas 10^U(lo, hi) per state - spec = [(lo, hi), (first, last, lo, hi), ...]: the default range, then ranges of blocks of
    states -, correlation from nfac common factors (the smaller `floor`, the stronger).  Element-wise sums only (no BLAS)."""
    lo, hi = np.full(30, float(spec[0][0])), np.full(30, float(spec[0][1]))
    for a, b, l, h in spec[1:]:
        lo[a:b], hi[a:b] = l, h
    sig = 10.0 ** rng.uniform(lo, hi)
    L = rng.normal(size=(30, nfac))
    Cm = floor * np.eye(30)
    for f in range(nfac):
        Cm = Cm + L[:, f][:, None] * L[:, f][None, :]
    s = sig / np.sqrt(np.diag(Cm))
    P = s[:, None] * Cm * s[None, :]
    return 0.5 * (P + P.T)


def correlated_prior(rng, lo, hi, nfac, floor):
    return block_prior(rng, [(lo, hi)], nfac, floor)


def crafted_record(rng, rec, x36, scales):
    """A kinematic + IMU record whose feet move by omega x foot_pos + foot_vel = scales[leg] * noise: feet with a small scale give rows that
    see the velocity alone, feet with a large one rows that see the rotation - otherwise the four feet's rows are near copies of each other
    and every pivot decision among them a near tie."""
    out = np.array(rec).copy()
    for leg in range(4):
        out["foot_vel"][leg] = -skew(x36[27:30]) @ out["foot_pos"][leg] + scales[leg] * rng.normal(size=3)
    return out


def plane_rows(rng, N, spread, rlo, rhi, rscale=1.0):
    """N rows [p x n, n] of points within 6 m that see (nearly) one plane: normals n0 + spread * noise."""
    n0 = rng.normal(size=3)
    n0 /= np.sqrt((n0 * n0).sum())
    n = n0 + spread * rng.normal(size=(N, 3))
    n /= np.sqrt((n * n).sum(axis=1, keepdims=True))
    p = rng.uniform(-6, 6, size=(N, 3))
    h6 = np.concatenate([np.cross(p, n), n], axis=1)
    z = rng.normal(0, 0.02, N)
    R = rscale * 10.0 ** rng.uniform(rlo, rhi, N)
    return h6, z, R


def state_at_origin(rng):
    """A state whose 27 additive components are 0: the posterior's ARE the state step, with no rounding of x + dx in between."""
    x = np.zeros(36)
    x[:9] = rodrigues(rng.normal(size=3)).reshape(-1)
    return x


# ----------------------------------------------------------------------------- the numpy restatement of the elimination (NOT the code under test)
VARIANTS = ("no_pivot", "rhs_not_swapped", "last_column_left", "search_from_row_0", "signed_pivot", "adjacent_skipped", "unpermuted_diagonal")


def gauss_jordan(S, G, variant=None):
    """X = S^-1 G by Gauss-Jordan with partial pivoting as dev_solve does it (first largest magnitude at or below the diagonal, whole rows of
    [S | G] swapped, all other rows eliminated, the division by the diagonal last) -> X, [(k, p)].  `variant` names one of the mistakes of
    VARIANTS; each is a line or two."""
    S, G = np.array(S, dtype=np.float64), np.array(G, dtype=np.float64)
    M = len(S)
    swaps, where = [], np.arange(M)
    for k in range(M):
        lo = 0 if variant == "search_from_row_0" else k
        col = S[lo:, k] if variant == "signed_pivot" else np.abs(S[lo:, k])
        p = lo + int(np.argmax(col))
        if variant == "no_pivot" or (variant == "adjacent_skipped" and p == k + 1):
            p = k
        if p != k:
            swaps.append((k, p))
            S[[k, p]] = S[[p, k]]
            where[[k, p]] = where[[p, k]]
            if variant != "rhs_not_swapped":
                last = G.shape[1] - 1 if variant == "last_column_left" else G.shape[1]
                G[[k, p], :last] = G[[p, k], :last]
        fac = S[:, k] / S[k, k]
        fac[k] = 0.0
        S -= fac[:, None] * S[k][None, :]
        G -= fac[:, None] * G[k][None, :]
    d = np.diag(S)
    if variant == "unpermuted_diagonal":
        d = d[where]
    return G / d[:, None], swaps


def mm(a, b):
    """a @ b with every sum taken term by term in index order, by element-wise products and sums alone: the same bits on every machine
    (a BLAS picks its summation order by the CPU it finds), which the measured constant below relies on."""
    a, b = np.atleast_2d(a), np.asarray(b)
    vec = b.ndim == 1
    b = b[:, None] if vec else b
    s = np.zeros((a.shape[0], b.shape[1]))
    for k in range(a.shape[1]):
        s = s + a[:, k][:, None] * b[k][None, :]
    return s[:, 0] if vec else s


def point_system(P, h6, z, R, eps_rule="reference"):
    """A, b of eskf.cc:91-113 in the information form; N == 1 adds 1e-4 to R (eskf.cc:98-104).  eps_rule: "never" / "always" are mistakes."""
    N = len(z)
    r = R + 0.0001 if (eps_rule == "always" or (eps_rule == "reference" and N == 1)) else R
    hr = h6 / r[:, None]
    A, b = mm(hr.T, h6), mm(hr.T, z)
    return np.eye(6) + mm(A, P[:6, :6]), np.concatenate([mm(A, P[:6, :]), b[:, None]], axis=1)


def restate_points(P, h6, z, R, variant=None, eps_rule="reference"):
    """-> dx (30), P' (30 x 30), swaps: dev_point_update in float64 numpy."""
    S, G = point_system(P, h6, z, R, eps_rule)
    X, swaps = gauss_jordan(S, G, variant)
    return mm(P[:, :6], X[:, 30]), P - mm(P[:, :6], X[:, :30]), swaps


def restate_dense(P, H, z, R, variant=None):
    """-> dx, P', swaps: dev_dense_update (S = H P H^T + R, G = [H P | z]) in float64 numpy."""
    PHT = mm(P, H.T)
    X, swaps = gauss_jordan(mm(H, PHT) + np.diag(R), np.concatenate([mm(H, P), z[:, None]], axis=1), variant)
    return mm(PHT, X[:, 30]), P - mm(PHT, X[:, :30]), swaps


# ----------------------------------------------------------------------------- 50 digits
def M_(a):
    """float64 array -> mpmath matrix, exactly."""
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix(a.tolist()) if a.ndim == 2 else mp.matrix([[float(v)] for v in a])


def to_f64(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def norm_inf(m):
    return max(sum(abs(m[i, j]) for j in range(m.cols)) for i in range(m.rows))


def exact_pivots(S):
    """The elimination on the 50-digit S -> [(k, p)], the smallest winner / runner-up ratio over all pivot decisions, and the smallest
    magnitude on the diagonal BEFORE pivoting."""
    S = S.copy()
    M = S.rows
    swaps, margin = [], mpf("inf")
    diag_min = min(abs(S[i, i]) for i in range(M))
    for k in range(M):
        mag = [abs(S[i, k]) for i in range(k, M)]
        p = k + max(range(M - k), key=lambda i: mag[i])
        if M - k > 1:
            margin = min(margin, mag[p - k] / max(max(v for i, v in enumerate(mag) if i != p - k), mpf(10) ** -300))
        if p != k:
            swaps.append((k, p))
            for c in range(M):
                S[k, c], S[p, c] = S[p, c], S[k, c]
        for i in range(M):
            if i != k:
                f = S[i, k] / S[k, k]
                for c in range(M):
                    S[i, c] -= f * S[k, c]
    return swaps, float(margin), float(diag_min)


def exp3_mp(v):
    """Exp of a rotation vector at 50 digits (Rodrigues; the series below 1e-20)."""
    x, y, z = v
    K = mp.matrix([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    n = mp.sqrt(x * x + y * y + z * z)
    if n < mpf(10) ** -20:
        return mp.eye(3) + K + K * K / 2
    return mp.eye(3) + (mp.sin(n) / n) * K + ((1 - mp.cos(n)) / (n * n)) * (K * K)


def _finish(P, PHT, S, HP, zc, extra):
    Sinv = S ** -1
    kappa = float(norm_inf(S) * norm_inf(Sinv))
    X = Sinv * HP
    Pn = P - PHT * X
    dx = PHT * (Sinv * zc)
    swaps, margin, diag_min = exact_pivots(S)
    out = dict(P=to_f64(Pn), dx=to_f64(dx)[:, 0], kappa=kappa, swaps=swaps, margin=margin, diag_min=diag_min, S=S, P_mp=Pn, dx_mp=dx,
               E=to_f64(exp3_mp([dx[0, 0], dx[1, 0], dx[2, 0]])))
    out.update(extra)
    return out


def ref_points(P, h6, z, R):
    """The point update at 50 digits from the float64 inputs: A = sum h h^T / R, b = sum h z / R (N == 1: R + 1e-4), then
    P' = P - P[:,0:6] (I + A P66)^-1 A P[0:6,:] and dx = P[:,0:6] (I + A P66)^-1 b.  For N <= 7 also the literal K = P H^T (H P H^T + R)^-1;
    the two agree to 1e-40.  `kappa_literal` is kappa_inf of the N x N system H P H^T + R, which the literal form answers for: at 50 digits up to
    N = 65, from numpy's float64 inverse at N = 300 (a 300 x 300 inverse at 50 digits takes minutes; kappa is 1e7 at most there, so float64
    gives it to nine digits)."""
    N = len(z)
    Pm, h = M_(P), M_(h6)
    r = [mpf(float(v)) + (mpf(0.0001) if N == 1 else 0) for v in R]
    A, b = mp.zeros(6, 6), mp.zeros(6, 1)
    for k in range(N):
        for i in range(6):
            hi = h[k, i] / r[k]
            for j in range(6):
                A[i, j] += hi * h[k, j]
            b[i, 0] += hi * mpf(float(z[k]))
    P6, P66 = Pm[0:6, 0:30], Pm[0:6, 0:6]
    out = _finish(Pm, Pm[0:30, 0:6], mp.eye(6) + A * P66, A * P6, b, {})
    if N <= 65:
        Hm = mp.zeros(N, 30)
        for k in range(N):
            for i in range(6):
                Hm[k, i] = h[k, i]
        SL = Hm * Pm * Hm.T
        for k in range(N):
            SL[k, k] += r[k]
        SLinv = SL ** -1
        out["kappa_literal"] = float(norm_inf(SL) * norm_inf(SLinv))
        if N <= 7:
            K = Pm * Hm.T * SLinv
            dP = norm_inf(Pm - K * Hm * Pm - out["P_mp"])
            ddx = norm_inf(K * M_(z) - out["dx_mp"])
            assert dP <= mpf(10) ** -40 and ddx <= mpf(10) ** -40, (float(dP), float(ddx))
    else:
        SL = mm(mm(h6, P[:6, :6]), h6.T) + np.diag(R)
        out["kappa_literal"] = float(np.abs(SL).sum(1).max() * np.abs(np.linalg.inv(SL)).sum(1).max())
    return out


def ref_dense(P, H, z, R):
    """K = P H^T (H P H^T + R)^-1 at 50 digits: P' = P - K H P, dx = K z."""
    Pm, Hm = M_(P), M_(H)
    PHT = Pm * Hm.T
    S = Hm * PHT
    for a in range(len(z)):
        S[a, a] += mpf(float(R[a]))
    return _finish(Pm, PHT, S, Hm * Pm, M_(z), {})


def kin_rows_mp(x36, rec, params, acc_norm=9.81):
    """msgcases.kin_rows with every product and sum at 50 digits -> H (M x 30), z (M x 1) as mpmath matrices, not rounded."""
    x = [mpf(float(v)) for v in x36]
    Rm = mp.matrix(3, 3)
    for i in range(9):
        Rm[i // 3, i % 3] = x[i]
    sk = lambda v: mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])   # noqa: E731
    legs = [leg for leg in range(4) if rec["contact"][leg] != 0]
    M = 6 + 3 * len(legs)
    H, z = mp.zeros(M, 30), mp.zeros(M, 1)
    scale = mpf(float(params["gravity"] / acc_norm))     # the quotient the device takes in float64 on the host
    for i in range(3):
        H[i, 9 + i] = H[i, 18 + i] = H[3 + i, 12 + i] = H[3 + i, 21 + i] = 1
        z[i, 0] = scale * mpf(float(rec["acc"][i])) - x[24 + i] - x[15 + i]
        z[3 + i, 0] = mpf(float(rec["gyr"][i])) - x[27 + i] - x[18 + i]
    w = x[27:30]
    for idx, leg in enumerate(legs):
        r0 = 6 + 3 * idx
        fp = mp.matrix([mpf(float(v)) for v in rec["foot_pos"][leg]])
        fv = mp.matrix([mpf(float(v)) for v in rec["foot_vel"][leg]])
        wpv = sk(w) * fp + fv
        B0, B21, Rw = -(Rm * sk(wpv)), -(Rm * sk(fp)), Rm * wpv
        for r in range(3):
            for c in range(3):
                H[r0 + r, c], H[r0 + r, 21 + c] = B0[r, c], B21[r, c]
            H[r0 + r, 6 + r] = 1
            z[r0 + r, 0] = -x[12 + r] - Rw[r]
    return H, z


def ref_message(x36, P, rec, params, kind, acc_norm=9.81):
    """The update of one IMU (kind "imu": rows 0..5 alone) or kinematic + IMU message at the prior's own time (dt = 0: the two predicts in
    front of it change nothing), rows built from state and message at 50 digits."""
    H, z = kin_rows_mp(x36, rec, params, acc_norm)
    if kind == "imu":
        H, z = H[0:6, 0:30], z[0:6, 0:1]
    M = H.rows
    R = [params["imu_acc_meas_noise"], params["imu_acc_meas_noise"], params["imu_acc_z_meas_noise"]] + [params["imu_gyr_meas_noise"]] * 3
    R = R + [params["kin_meas_noise"]] * (M - 6)
    Pm = M_(P)
    PHT = Pm * H.T
    S = H * PHT
    for a in range(M):
        S[a, a] += mpf(float(R[a]))
    out = _finish(Pm, PHT, S, H * Pm, z, {})
    out["x_add"] = np.array([float(mpf(float(x36[9 + i])) + out["dx_mp"][3 + i, 0]) for i in range(27)])    # x (+) dx at 50 digits, rounded once
    return out


# ----------------------------------------------------------------------------- the criterion
def bounds(ref, P_prior, c):
    """-> (covariance bound, state-step bound) of the criterion for a result compared with `ref`."""
    return c * EPS * ref["kappa"] * np.abs(P_prior).max(), c * EPS * ref["kappa"] * np.abs(ref["dx"]).max()


def ratios(ref, P_prior, dx, Pn, kappa=None):
    """err / (EPS * kappa * scale) of a result: covariance, state step, asymmetry (against TWICE the covariance scale, so that one c serves)."""
    k = ref["kappa"] if kappa is None else kappa
    sP, sx = EPS * k * np.abs(P_prior).max(), EPS * k * np.abs(ref["dx"]).max()
    return np.abs(Pn - ref["P"]).max() / sP, np.abs(dx - ref["dx"]).max() / sx, np.abs(Pn - Pn.T).max() / (2 * sP)


def rotation_step(x_prior, x_post):
    return x_prior[:9].reshape(3, 3).T @ x_post[:9].reshape(3, 3)


# what a 3 x 3 product of rotation entries, the device's own Exp (sin, cos, a division, two 3 x 3 products) and the product with the prior
# can lose in float64 on entries of magnitude <= 1: a few dozen half-ulps of 1, independent of the solve.  Exp is 1-Lipschitz in the
# entries (up to sqrt 2), so the state-step bound of the three rotation components carries over with a factor 2.
ROT_FLOOR = 64 * EPS


def rotation_bound(dx_bound):
    return 2 * dx_bound + ROT_FLOOR


# ----------------------------------------------------------------------------- the case table (outcome of the seeded search, frozen)
GEN_A = (-4, -1.5, 2, 0.05, 0.05, -4, -3)      # sigma range 10^lo .. 10^hi, factors, floor, spread of the normals, R range 10^rlo .. 10^rhi
GEN_B = (-2.5, 0, 2, 0.05, 0.05, -4, -3)
GEN_C = (-3.5, -1, 2, 0.02, 0.05, -3.5, -3)
GEN_D = (-3, 0, 3, 0.1, 0.1, -5, -3)
GEN_E = (-4, 0, 2, 0.05, 0.02, -5, -3)
GEN_F = (-3.5, -1.5, 3, 0.05, 0.3, -4, -3)

# name: (N, seed, generator, scale of R, swaps under exact arithmetic, kappa_inf(S) <= 1e3)
POINT_TABLE = {
    "k0_n6": (6, 28, GEN_A, 1.0, [(0, 2)], True),
    "k1_n2": (2, 1215, (-1.5, 0, 1, 0.05, 0.05, -3.3, -3), 1.0, [(1, 4)], True),
    "k2_n6": (6, 311, GEN_C, 1.0, [(2, 5)], True),
    "k3_n7": (7, 555, GEN_A, 1.0, [(3, 5)], True),
    "k4_adjacent_n64": (64, 962, (-4, -2, 1, 0.02, 0.03, -3.5, -3), 1.0, [(4, 5)], True),
    "adjacent_n3": (3, 188, GEN_A, 1.0, [(1, 2)], True),
    "distant_n1": (1, 1056, GEN_B, 1.0, [(0, 5)], True),
    "distant_n1_b": (1, 1056, GEN_E, 1.0, [(0, 5)], True),
    "two_swaps_n64": (64, 282, GEN_A, 1.0, [(0, 3), (1, 2)], True),
    "three_swaps_n65": (65, 466, GEN_C, 1.0, [(0, 1), (2, 5), (3, 5)], True),
    "row_moves_twice_n2": (2, 1326, GEN_F, 1.0, [(0, 1), (1, 2)], True),
    "control_n300": (300, 156, GEN_A, 1.0, [], True),
    "n1_swap": (1, 404, GEN_B, 1.0, [(0, 1)], True),
    "n1_control": (1, 312, GEN_D, 1.0, [], True),
    "small_diagonal_n3": (3, 67, GEN_D, 7.455195196233071, [(0, 2)], True),
    "small_diagonal_adjacent_n3": (3, 105, GEN_A, 2.4672155601244805, [(0, 1)], True),
    "small_diagonal_negative_n3": (3, 4916, GEN_C, 0.37788997087028825, [(0, 1)], False),      # ... and every other entry of column 0 negative
    "two_swaps_n300": (300, 282, GEN_A, 1.0, [(0, 3), (1, 2)], False),
    "n2_hi": (2, 250, GEN_B, 1.0, [(0, 1)], False),
    "n3_hi_two": (3, 384, GEN_B, 1.0, [(0, 1), (1, 3)], False),
    "n3_hi": (3, 279, GEN_B, 1.0, [(0, 1)], False),
    "n6_hi_two": (6, 616, GEN_B, 1.0, [(1, 2), (2, 4)], False),
    "n6_hi": (6, 784, GEN_B, 1.0, [(0, 2)], False),
    "n7_hi_two": (7, 1011, GEN_B, 1.0, [(0, 1), (1, 2)], False),
    "n7_hi": (7, 304, GEN_B, 1.0, [(1, 2)], False),
    "n64_hi_three": (64, 914, GEN_B, 1.0, [(0, 1), (1, 2), (2, 3)], False),
    "n64_hi": (64, 232, GEN_B, 1.0, [(0, 2)], False),
    "n65_hi_four": (65, 677, GEN_B, 1.0, [(0, 1), (1, 5), (2, 5), (3, 5)], False),
    "n65_hi_three": (65, 914, GEN_B, 1.0, [(0, 1), (1, 2), (2, 3)], False),
    "n300_hi_two": (300, 1095, GEN_D, 1.0, [(3, 5), (4, 5)], False),
}
SMALL_DIAGONAL = ("small_diagonal_n3", "small_diagonal_adjacent_n3", "small_diagonal_negative_n3")     # R scaled so that S[0][0] = 1 + (A P66)[0][0] is 1e-7

# name: (index of the record in msgcases.one_message_per_mask (contact mask 0 asked of it: IMU rows alone), seed, prior generator, swaps, low)
IMU_TABLE = {
    "imu_adjacent": (0, 292, (-2, -0.5, 2, 0.05), [(3, 4)], True),
    "imu_k0": (1, 610, (-2.5, 0.5, 1, 0.02), [(0, 3)], True),
    "imu_two": (2, 530, (-2, 0, 2, 0.02), [(0, 4), (1, 3)], True),
    "imu_distant_two": (3, 79, (-2, -0.5, 2, 0.05), [(0, 5), (4, 5)], True),
    "imu_three": (4, 736, (-1, 0.5, 2, 0.2), [(0, 3), (1, 4), (3, 4)], True),
    "imu_five": (5, 98, (-1, 1, 3, 0.05), [(0, 5), (1, 5), (2, 4), (3, 4), (4, 5)], False),
    "imu_three_hi": (6, 201, (-1, 1, 3, 0.05), [(1, 2), (2, 5), (3, 5)], False),
    "imu_distant_hi": (7, 425, (-2.5, 0.5, 1, 0.02), [(0, 5)], False),
}

LATE = [(-3, -2), (0, 3, -0.5, 0.7), (6, 9, -0.8, -0.4), (21, 24, -3, -2)]     # rotation sigmas 0.3 .. 5, velocity 0.16 .. 0.4, everything else small
# name: (contact mask, seed, prior generator (4 numbers: correlated_prior; else block spec + factors + floor), foot scales of crafted_record or None, swaps)
DENSE_TABLE = {
    "m6_four": (0, 711, (-1, 0.5, 2, 0.2), None, [(0, 5), (1, 3), (2, 5), (4, 5)]),
    "m6_one": (0, 687, (-2, 0, 2, 0.02), None, [(0, 2)]),
    "m9_four": (1, 761, (-2, 0, 2, 0.02), None, [(0, 7), (1, 4), (3, 4), (5, 7)]),
    "m9_two": (4, 678, (-1, 0.5, 2, 0.2), None, [(0, 7), (3, 7)]),
    "m12_four": (3, 200, (-2, 0, 2, 0.02), None, [(0, 4), (1, 5), (3, 4), (4, 5)]),
    "m12_one": (10, 610, (-2.5, 0.5, 1, 0.02), None, [(0, 3)]),
    "m15_three": (7, 97, (-1.5, 0.5, 2, 0.05), None, [(0, 1), (1, 4), (3, 4)]),
    "m15_adjacent": (13, 712, (-1, 0.5, 2, 0.2), None, [(1, 2)]),
    "m18_late_four": (15, 375, (LATE, 3, 10.0), (0.01, 0.01, 0.3, 1), [(4, 17), (12, 15), (13, 17), (14, 17)]),
    "m18_late_three": (15, 2000, (LATE, 3, 10.0), (0.01, 0.01, 0.1, 2), [(3, 17), (14, 17), (15, 17)]),
    "m18_four": (15, 2251, (-1.5, 0.5, 2, 0.05), None, [(0, 2), (1, 4), (2, 4), (3, 4)]),
    "m18_two": (15, 2199, (-2, 0, 2, 0.02), None, [(0, 5), (1, 3)]),
}
T_MSG = 1.0      # stamp of the records (and time of the priors in the message tests)


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def message_base():
    """-> scene, the state the dense rows are built at, 16 records (one per contact mask) at T_MSG."""
    sc = mc.scene()
    x = synth.initial_state(sc.traj, T_MSG, sc.P)
    x[15:21] = np.random.default_rng(8).normal(0, 0.01, 6)
    return sc, x, mc.one_message_per_mask(sc, T_MSG)


def at_origin(x_rows):
    x = np.zeros(36)
    x[:9] = x_rows[:9]
    return x


@functools.lru_cache(maxsize=None)
def point_case(name):
    N, seed, gen, rscale, swaps, low = POINT_TABLE[name]
    rng = np.random.default_rng(seed)
    P = correlated_prior(rng, *gen[:4])
    h6, z, R = plane_rows(rng, N, gen[4], gen[5], gen[6], rscale)
    return Case(name=name, kind="points", N=N, x36=state_at_origin(rng), P=P, h6=h6, z=z, R=R, swaps=swaps, low=low)


@functools.lru_cache(maxsize=None)
def imu_case(name):
    idx, seed, gen, swaps, low = IMU_TABLE[name]
    sc, x_rows, kins = message_base()
    rec = np.array(kins[idx]).copy()
    rec["contact"][:] = 0
    H, z, R = mc.kin_rows(x_rows, rec, sc.P)
    P = correlated_prior(np.random.default_rng(seed), *gen)
    return Case(name=name, kind="imu", x_rows=x_rows, x36=at_origin(x_rows), P=P, rec=rec, H=H, z=z, R=R, swaps=swaps, low=low)


@functools.lru_cache(maxsize=None)
def dense_case(name):
    mask, seed, gen, scales, swaps = DENSE_TABLE[name]
    sc, x_rows, kins = message_base()
    rng = np.random.default_rng(seed)
    rec = np.array(kins[mask]).copy()
    if scales is not None:
        rec = crafted_record(rng, rec, x_rows, scales)
    P = block_prior(rng, *gen) if len(gen) == 3 else correlated_prior(rng, *gen)
    H, z, R = mc.kin_rows(x_rows, rec, sc.P)
    assert mc.masks_of(rec[None])[0] == mask and len(z) == 6 + 3 * bin(mask).count("1")
    return Case(name=name, kind="dense", mask=mask, x_rows=x_rows, x36=at_origin(x_rows), P=P, rec=rec, H=H, z=z, R=R, swaps=swaps, low=None)


def all_cases():
    return [point_case(n) for n in POINT_TABLE] + [imu_case(n) for n in IMU_TABLE] + [dense_case(n) for n in DENSE_TABLE]


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    c = {"points": point_case, "imu": imu_case, "dense": dense_case}[kind](name)
    return ref_points(c.P, c.h6, c.z, c.R) if kind == "points" else ref_dense(c.P, c.H, c.z, c.R)


def reference(c):
    """The 50-digit result of a table case (computed once per process)."""
    return _reference(c.kind, c.name)


def moved_twice(swaps, M):
    """Some row of the original system takes part in two swaps."""
    count, where = {}, list(range(M))
    for k, p in swaps:
        for r in (where[k], where[p]):
            count[r] = count.get(r, 0) + 1
        where[k], where[p] = where[p], where[k]
    return max(count.values(), default=0) >= 2


def kinds_of(swaps, M=6):
    """The kinds of swap the issue lists, as a set of names."""
    out = {f"k{k}" for k, _ in swaps if k < 5}
    out |= {"adjacent"} if any(p == k + 1 for k, p in swaps) else set()
    out |= {"distant"} if (0, 5) in swaps else set()
    out |= {{0: "control", 2: "two", 3: "three"}.get(len(swaps), "other")}
    out |= {"twice"} if moved_twice(swaps, M) else set()
    return out - {"other"}


POINT_KINDS = {"k0", "k1", "k2", "k3", "k4", "adjacent", "distant", "two", "three", "twice", "control"}


def assert_case(c, ref=None):
    """What the table states of a case, on its 50-digit system: the swap list, every pivot decision clear by MARGIN, kappa within the caps."""
    ref = reference(c) if ref is None else ref
    assert ref["swaps"] == c.swaps, (c.name, ref["swaps"], c.swaps)
    assert ref["margin"] >= MARGIN, (c.name, ref["margin"])
    assert ref["kappa"] <= (KAPPA_LOW if c.low else KAPPA_CAP), (c.name, ref["kappa"])
    assert np.array_equal(c.P, c.P.T) and np.linalg.eigvalsh(c.P).min() > 0, c.name
    if c.kind == "points":
        assert len(c.z) == c.N and c.N in (1, 2, 3, 6, 7, 64, 65, 300)
        if c.N == 1:
            assert 1e-5 <= c.R[0] <= 1e-3, (c.name, c.R)       # the scale r / (r + 1e-4) is between 0.09 and 0.91
    if c.name in SMALL_DIAGONAL:
        assert ref["diag_min"] < 0.1, ref["diag_min"]


def assert_table():
    """What the table as a whole promises."""
    pts = [point_case(n) for n in POINT_TABLE]
    low = [c for c in pts if c.low]
    assert 3 * len(low) >= len(pts), (len(low), len(pts))
    seen = set().union(*(kinds_of(c.swaps) for c in low))
    assert seen >= POINT_KINDS, POINT_KINDS - seen
    assert {c.N for c in pts} == {1, 2, 3, 6, 7, 64, 65, 300}
    assert any(c.N == 1 and c.swaps for c in pts) and any(c.N == 1 and not c.swaps for c in pts)
    dense = [dense_case(n) for n in DENSE_TABLE]
    assert {len(c.z) for c in dense} == {6, 9, 12, 15, 18}
    assert any(len(c.z) == 18 and any(k >= 12 for k, _ in c.swaps) for c in dense) and any(len(c.z) == 18 and len(c.swaps) >= 4 for c in dense)
    assert all(c.swaps for c in dense) and all(imu_case(n).swaps for n in IMU_TABLE)


# ----------------------------------------------------------------------------- the measured constant
# Largest err / (EPS * kappa * scale) of restate_points / restate_dense over the table (inputs of the fixture; sums in index order, see mm):
# covariance 0.107 (k4_adjacent_n64), state step 0.534 (k4_adjacent_n64, kappa 31: at a small kappa the products around the solve weigh most),
# asymmetry 0.064.  One constant for the three, as the criterion has one c.
RATIO_MEASURED = 0.535
C = 16 * RATIO_MEASURED      # 8.56


# ----------------------------------------------------------------------------- the fixture: inputs and 50-digit results, rounded to float64
IU = np.triu_indices(30)


def pack_sym(Pm):
    return np.ascontiguousarray(Pm[IU])


def unpack_sym(v):
    Pm = np.zeros((30, 30))
    Pm[IU] = v
    return Pm + np.triu(Pm, 1).T


def message_reference(c):
    sc = message_base()[0]
    return ref_message(c.x_rows, c.P, c.rec, sc.P, "imu" if c.kind == "imu" else "kin")


def full_reference(c):
    return ref_points(c.P, c.h6, c.z, c.R) if c.kind == "points" else ref_dense(c.P, c.H, c.z, c.R)


def expected_arrays(c, ref=None, with_message=True):
    """The fixture's entries of one case from its inputs: the 50-digit posterior, step, Exp of the step's rotation part and kappa."""
    ref = full_reference(c) if ref is None else ref
    out = {"P50": pack_sym(ref["P"]), "dx50": ref["dx"], "E50": ref["E"], "kappa": np.array([ref["kappa"], ref.get("kappa_literal", 0.0)])}
    if c.kind != "points" and with_message:
        m = message_reference(c)
        out.update({"msg_P50": pack_sym(m["P"]), "msg_dx50": m["dx"], "msg_E50": m["E"], "msg_kappa": np.array([m["kappa"]]), "msg_xadd50": m["x_add"]})
    return out


def input_arrays(c):
    if c.kind == "points":
        return {"x36": c.x36, "P": pack_sym(c.P), "h6": c.h6, "z": c.z, "R": c.R}
    return {"x36": c.x36, "x_rows": c.x_rows, "P": pack_sym(c.P), "H": c.H, "z": c.z, "R": c.R, "rec": np.array(c.rec)}


def build_fixture():
    out = {}
    for c in all_cases():
        for k, v in {**input_arrays(c), **expected_arrays(c)}.items():
            out[f"{c.name}/{k}"] = v
    return out


def write_fixture():
    np.savez_compressed(GOLDEN, **build_fixture())


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def stored_case(name):
    """A table case with the inputs AND expected values of the fixture (what every test but the regeneration uses: the fixture's inputs are
    the case - a seed gives them to the last bit only where numpy's pow is the same)."""
    g = _golden()
    kind, table = next((k, t) for k, t in (("points", POINT_TABLE), ("imu", IMU_TABLE), ("dense", DENSE_TABLE)) if name in t)
    f = {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(name + "/")}
    c = Case(name=name, kind=kind, swaps=table[name][-2] if kind != "dense" else table[name][-1], low=table[name][-1] if kind != "dense" else None)
    c.x36, c.P, c.z, c.R = f["x36"], unpack_sym(f["P"]), f["z"], f["R"]
    if kind == "points":
        c.h6, c.N = f["h6"], len(f["z"])
    else:
        c.H, c.x_rows, c.rec = f["H"], f["x_rows"], f["rec"]
        c.msg = dict(P=unpack_sym(f["msg_P50"]), dx=f["msg_dx50"], E=f["msg_E50"], kappa=float(f["msg_kappa"][0]), x_add=f["msg_xadd50"])
    c.ref = dict(P=unpack_sym(f["P50"]), dx=f["dx50"], E=f["E50"], kappa=float(f["kappa"][0]), kappa_literal=float(f["kappa"][1]))
    return c


def stored_cases(kind):
    return [stored_case(n) for n in {"points": POINT_TABLE, "imu": IMU_TABLE, "dense": DENSE_TABLE}[kind]]


def check(name, ref, P_prior, dx, Pn, c=None, kappa=None, report=None):
    """The criterion for one result; prints each figure before it asserts.  -> the three ratios err / (EPS * kappa * scale)."""
    c = C if c is None else c
    r = ratios(ref, P_prior, dx, Pn, kappa)
    print(f"{name}: kappa {ref['kappa'] if kappa is None else kappa:.3g}  P {r[0]:.3g}  dx {r[1]:.3g}  asymmetry {r[2]:.3g}  (c = {c:.3g})")
    if report is not None:
        report.append((name,) + tuple(float(v) for v in r))
    assert r[0] <= c, (name, "covariance", r[0], c)
    assert r[1] <= c, (name, "state step", r[1], c)
    assert r[2] <= c, (name, "asymmetry", r[2], c)
    return r


def step_of(x_prior, x_post):
    """The 27 additive components of the state step (exact where the prior's are 0) and the rotation step R_prior^T R_post."""
    return x_post[9:] - x_prior[9:], rotation_step(x_prior, x_post)


def check_state(name, ref, x_prior, x_post, P_prior, Pn, c=None, kappa=None, report=None):
    """check() for a posterior held as a state: the additive components' step read off x_post (the prior's are 0 in every table case, so the
    difference is exact), its rotation part through R_prior^T R_post against Exp(dx_50[0:3]) within rotation_bound."""
    c = C if c is None else c
    add, E = step_of(x_prior, x_post)
    assert not np.any(x_prior[9:]), "the step is read exactly only from a prior whose additive components are 0"
    dx = np.concatenate([ref["dx"][:3], add])       # the three rotation components are judged through E below
    r = check(name, ref, P_prior, dx, Pn, c, kappa, report)
    k = ref["kappa"] if kappa is None else kappa
    rb = rotation_bound(c * EPS * k * np.abs(ref["dx"]).max())
    er = np.abs(E - ref["E"]).max()
    print(f"{name}: rotation step off by {er:.3g} (bound {rb:.3g})")
    assert er <= rb, (name, "rotation", er, rb)
    return r


def x_add_of(x_prior, ref):
    """The 27 additive components of x (+) dx_50, summed at 50 digits and rounded once."""
    return np.array([float(mpf(float(x_prior[9 + i])) + ref["dx_mp"][3 + i, 0]) for i in range(27)])


def check_posterior(name, ref, x_prior, x_post, P_prior, Pn, x_add, c=None, report=None):
    """The criterion for a posterior whose prior has additive components of its own (the states the map and the messages are seen from).
    The state step is then not readable exactly: x_post = fl(x + dx) carries half an ulp of ITS size, and x_add (x + dx_50 rounded once)
    another.  Those two half-ulps, 2 * EPS * |x_add| per component, are taken off the difference before it is held against the state-step
    bound - a property of the number format, not of the solve; covariance, asymmetry and rotation as in check_state."""
    c = C if c is None else c
    k = ref["kappa"]
    sP, sx = EPS * k * np.abs(P_prior).max(), EPS * k * np.abs(ref["dx"]).max()
    ex = np.maximum(np.abs(x_post[9:] - x_add) - 2 * EPS * np.abs(x_add), 0.0).max()
    r = (np.abs(Pn - ref["P"]).max() / sP, ex / sx, np.abs(Pn - Pn.T).max() / (2 * sP))
    er, rb = np.abs(rotation_step(x_prior, x_post) - ref["E"]).max(), rotation_bound(c * sx)
    print(f"{name}: kappa {k:.3g}  P {r[0]:.3g}  dx {r[1]:.3g}  asymmetry {r[2]:.3g}  (c = {c:.3g}); rotation step off by {er:.3g} (bound {rb:.3g})")
    if report is not None:
        report.append((name,) + tuple(float(v) for v in r))
    assert r[0] <= c, (name, "covariance", r[0], c)
    assert r[1] <= c, (name, "state step", r[1], c)
    assert r[2] <= c, (name, "asymmetry", r[2], c)
    assert er <= rb, (name, "rotation", er, rb)
    return r
