"""The synthetic room and trajectory moved AWAY from the origin, and plane fits judged against exact arithmetic.

Every other parity test runs in the room of legkilo_amd.synth as it stands: centred on the origin, floor at z = 0, root-voxel keys in
x [-41, 40], y [-31, 30], z [-2, 16], walls exactly on voxel faces.  PlacedWorld / PlacedTrajectory shift both by a vector D, so the
same scans, seeds and IMU / kinematic streams (accelerations, rates and velocities do not depend on D) arrive at world coordinates of
10^2 .. 10^5 m: negative keys on every axis, walls off the voxel faces, keys around +-6 000 and - `edge` - past the +-2^20 range of
the overlay's packed root keys.

Away from the origin the reference's plane refit (raw moments: sum p p^T / m - c c^T) carries an absolute error of about eps |p|^2, so
closed-loop runs of two implementations drift apart there ("Parity away from the origin").  plane_fit_errors judges each
fit on its own instead: against a centred two-pass fit of the same stored points in long double, with the first-order rounding bound
of sequentially summed raw moments as the bar.
"""
import numpy as np

import offconfig
from legkilo_amd import abi

PLACEMENTS = dict(
    origin=(0.0, 0.0, 0.0),                  # control
    negz=(-7.3, 4.1, -12.6),                 # every z key negative; conditioning as at the origin
    neg=(-100.3, -80.7, -40.2),              # all keys negative; walls off the voxel faces
    far=(3000.25, -2000.4, -150.1),          # keys around +-6 000
    edge=(600000.3, 70.2, -30.1),            # x keys ~1.2 M > 2^20: the packed-key range of the overlay only
)


class PlacedWorld:
    """world shifted by D: raycast(o, d) = world.raycast(o - D, d); lo / hi / slabs shifted."""

    def __init__(self, world, D):
        self.world, self.D = world, np.asarray(D, float)
        self.lo, self.hi = world.lo + self.D, world.hi + self.D
        self.slabs = world.slabs + np.repeat(self.D, 2)

    def raycast(self, o, d):
        return self.world.raycast(np.asarray(o, float) - self.D, d)


class PlacedTrajectory:
    """traj shifted by D: pos(t) + D; rot, vel, acc, omega_body are the inner trajectory's (finite differences of the SHIFTED position
    would lose |D| / h^2 * eps)."""

    def __init__(self, traj, D):
        self.traj, self.D = traj, np.asarray(D, float)

    def pos(self, t):
        return self.traj.pos(t) + self.D

    def rot(self, t):
        return self.traj.rot(t)

    def vel(self, t, *a, **k):
        return self.traj.vel(t, *a, **k)

    def acc(self, t, *a, **k):
        return self.traj.acc(t, *a, **k)

    def omega_body(self, t, *a, **k):
        return self.traj.omega_body(t, *a, **k)


def placed_scene(place, name=None, use_kin=False, **caps):
    """offconfig.scene(name, use_kin, **caps) with its world and trajectory moved to PLACEMENTS[place]."""
    sc = offconfig.scene(name, use_kin, **caps)
    D = PLACEMENTS[place]
    sc.world, sc.traj = PlacedWorld(sc.world, D), PlacedTrajectory(sc.traj, D)
    sc.place = place
    return sc


# ----------------------------------------------------------------------------- plane fits in long double
LD = np.longdouble


def _eigh3_ld(A):
    """Eigenvalues (ascending) and eigenvectors (columns) of a symmetric 3 x 3 long-double matrix: cyclic Jacobi, run to a fixed point."""
    A = np.array(A, dtype=LD)
    V = np.eye(3, dtype=LD)
    for _ in range(60):
        off = abs(A[0, 1]) + abs(A[0, 2]) + abs(A[1, 2])
        if off == 0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p, q] == 0:
                continue
            with np.errstate(over="ignore"):     # an off-diagonal entry at the underflow level: theta = inf, t = 0
                theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = np.sign(theta) / (abs(theta) + np.hypot(theta, LD(1))) if theta != 0 else LD(1)
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            J = np.eye(3, dtype=LD)
            J[p, p] = J[q, q] = c
            J[p, q], J[q, p] = s, -s
            A = J.T @ A @ J
            A[p, q] = A[q, p] = 0
            V = V @ J
    w = np.array([A[0, 0], A[1, 1], A[2, 2]], dtype=LD)
    order = np.argsort(w)
    return w[order], V[:, order]


def fit_plane_ld(pw):
    """Centred two-pass fit of (m, 3) points in long double -> (centre, unit normal, eigenvalues ascending)."""
    p = np.asarray(pw).astype(LD)
    c = p.sum(0) / LD(len(p))
    q = p - c
    w, V = _eigh3_ld(q.T @ q / LD(len(p)))
    return c, V[:, 0], w


def plane_fit_errors(blob):
    """For every plane node of a blob whose point block is present: the stored normal and centre against the long-double fit of the
    first `points_size` stored points (the points the plane was last fitted on; later ones wait for the next refit).
    -> arrays (normal error up to sign, centre error, B), B = (m + 4) 2^-53 max|p|^2 / (lambda_mid - lambda_min): the first-order
    rounding bound on the normal of a fit from raw moments summed sequentially over m points in double."""
    b = abi.parse_blob(blob)
    nodes, planes, blocks = b["nodes"], b["planes"], b["blocks"]
    en, ec, B = [], [], []
    for i in np.flatnonzero((planes["flags"] & abi.LK_PLANE_IS_PLANE) != 0):
        n, pl = nodes[i], planes[i]
        m = int(pl["points_size"])
        if n["block"] < 0 or n["npts"] <= 0 or m > int(n["npts"]) or m < 3:
            continue
        pw = blocks[int(n["block"])]["pts"]["pw"][:m]
        c, nrm, w = fit_plane_ld(pw)
        got_n, got_c = np.asarray(pl["normal"]).astype(LD), np.asarray(pl["center"]).astype(LD)
        en.append(float(min(np.sqrt(((got_n - nrm) ** 2).sum()), np.sqrt(((got_n + nrm) ** 2).sum()))))
        ec.append(float(np.abs(got_c - c).max()))
        B.append(float(LD(m + 4) * LD(2.0) ** -53 * (pw.astype(LD) ** 2).sum(1).max() / (w[1] - w[0])))
    return np.array(en), np.array(ec), np.array(B)
