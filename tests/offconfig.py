"""Named configurations AWAY from the shipped yaml files, and the crafted scenes that go with them.

Every key lk_create accepts beyond the shipped values - a tilted, not exactly orthonormal extrinsic rotation, a voxel size that
is no power of two, tree depths 0 .. 4 with per-layer thresholds that differ, a freeze before the point block is full, other gate
constants - is run by tests/test_config_space.py (HIP vs oracle) after tests/test_reference_pin.py has pinned the oracle against
the reference's own build at the SAME entries of this table.  All generators are seeded.
"""
import numpy as np

import oracle_binding as ob
import scenes
from legkilo_amd import config, synth

# yaml-style 6 decimals: NOT exactly orthonormal, as a calibration file would give it
TILT_R = [float(v) for v in np.round(ob.exp_log(np.array([0.35, -0.2, 2.4]))[0], 6).reshape(9)]

_TILT = dict(extrinsic_R=TILT_R, extrinsic_T=[0.12, -0.03, 0.25])
_VS04 = dict(voxel_size=0.4)
_LAYERS3 = dict(max_layer=3, layer_init_num=[5, 6, 7, 8, 9], max_points_num=30)

CONFIGS = dict(
    tilt=_TILT,
    vs04=_VS04,
    layers3=_LAYERS3,
    layer0=dict(max_layer=0, layer_init_num=[8, 5, 5, 5, 5], max_points_num=20),
    all=dict(_TILT, **_VS04, **_LAYERS3, sigma_num=2.5, beam_err=0.3, dept_err=0.03),
    # crafted scenes only: with min_eigen_value = 5e-5 the synthetic world's walls (2 cm noise) are no planes at all
    deep4=dict(max_layer=4, min_eigen_value=5e-5, layer_init_num=[5, 6, 7, 8, 9], max_points_num=30),
    deep3=dict(max_layer=3, voxel_size=0.4, min_eigen_value=5e-5, layer_init_num=[5, 6, 7, 8, 9], max_points_num=30),
    # thresholds that FALL with depth: a child can be due for its first fit with fewer points than the root needed (every other entry rises)
    desc4=dict(max_layer=4, min_eigen_value=5e-5, layer_init_num=[9, 8, 7, 6, 5], max_points_num=30),
    # -0.0 != the bit pattern of the identity: the handle takes the generic kernels, with identity arithmetic
    negzero=dict(extrinsic_R=[1, -0.0, 0, 0, 1, 0, 0, 0, 1]),
)
CLOSED_LOOP = ("tilt", "vs04", "layers3", "layer0", "all")
CRAFTED = ("deep4", "deep3", "desc4")


def params(name, use_kin=False):
    """Parameter dict of a named configuration on top of LEG_FUSION (IMU-only) or DITER with the 0.3 m voxel grid (leg fusion)."""
    base = dict(config.DITER, voxel_grid_resolution=0.3) if use_kin else dict(config.LEG_FUSION)
    if name is not None:
        base.update(CONFIGS[name])
    return base


def scene(name, use_kin=False, **caps):
    return scenes.Scene(params=params(name, use_kin), **caps)


# ----------------------------------------------------------------------------- raw scans with z == 0 points
class ZeroZ:
    """scenes.vlp_scan_input with z = 0 forced on every 37th raw point: calcBodyCov's z == 0 guard (voxel_map.cc:23) on the path.
    Counts the path points (after the voxel grid) that still have z == 0 exactly."""

    def __init__(self):
        self.n_zero = 0
        self.n_pts = 0

    def __call__(self, scene_, tb, k):
        P = scene_.P
        raw = synth.vlp16_scan(scene_.world, scene_.traj, tb, P, seed_noise=3003 + k)
        raw["z"][::37] = 0.0
        pre = synth.preprocess_velodyne(raw, P["filter_num"], P["blind"])
        ds = synth.sort_by_time(synth.voxel_grid_centroid(pre, P["voxel_grid_resolution"]))
        self.n_zero += int((ds["z"] == 0.0).sum())
        self.n_pts += len(ds)
        return ds


# ----------------------------------------------------------------------------- crafted scenes
BOX_LO, BOX_HI = np.array([4.0, 4.0, 0.5]), np.array([5.0, 4.5, 1.0])
CHUNKS = (1, 1, 5, 17, 200, 1000, 5000)       # then the rest


def chunks_of(n, sizes=CHUNKS):
    """[a, b) ranges: the sizes in turn, then whatever is left."""
    out, k = [], 0
    for c in sizes:
        if k >= n:
            break
        out.append((k, min(n, k + c)))
        k = out[-1][1]
    if k < n:
        out.append((k, n))
    return out


def uniform_box(seed, n=40000, offset=(0.0, 0.0, 0.0)):
    """Volumetric clutter uniform in the box [4, 5] x [4, 4.5] x [0.5, 1]: nothing but non-planes, cut down to max_layer.
    -> (world points f64, variance rows)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(BOX_LO, BOX_HI, (n, 3)) + np.asarray(offset, float)
    var = np.tile((np.eye(3) * 4e-4).reshape(1, 9), (n, 1))
    return p, var


class CornerSites:
    """Three mutually perpendicular thin sheets over the box (one coordinate = 4.37 / 4.21 / 0.71 + N(0, 1 mm)), replicated at
    `n_sites` random offsets so that the crease lines fall off the voxel faces and a launch has many root voxels to work on.
    Near a crease a voxel holds two or three sheets (no plane: cut), away from it one (a plane): planes and matches on every
    layer of a deep tree.  points() are the map points (variance 1e-6 I); fresh(seed) draws new points on the same sheets, 2 mm off
    (variance 1e-5 I), for queries and inserted scans."""

    LEVELS = (4.37, 4.21, 0.71)

    def __init__(self, seed, n_sites=1, per_sheet=12000):
        rng = np.random.default_rng(seed)
        self.seed, self.per_sheet = seed, per_sheet
        offs = [np.zeros(3)]
        grid = rng.permutation(64)[: n_sites - 1]
        for g in grid:   # distinct cells of a 2.5 m lattice (sites never share a root voxel), random sub-voxel shift inside
            cell = np.array([g % 8 - 4, (g // 8) % 8 - 4, 0.0]) * 2.5 + [12.0, -3.0, 0.0]
            offs.append(cell + np.r_[rng.uniform(0, 0.5, 2), rng.uniform(0, 0.5)])
        self.offsets = np.array(offs[:n_sites])

    def _draw(self, rng, n, sigma):
        out = []
        for off in self.offsets:
            for ax in range(3):
                p = rng.uniform(BOX_LO, BOX_HI, (n, 3))
                p[:, ax] = self.LEVELS[ax] + rng.normal(0, sigma, n)
                out.append(p + off)
        p = np.concatenate(out)
        rng.shuffle(p)
        return p

    def points(self):
        p = self._draw(np.random.default_rng(self.seed + 1), self.per_sheet, 0.001)
        return p, np.tile((np.eye(3) * 1e-6).reshape(1, 9), (len(p), 1))

    def fresh(self, seed, n_per_sheet=700):
        p = self._draw(np.random.default_rng(self.seed + 1000 + seed), n_per_sheet, 0.002)
        return p, np.tile((np.eye(3) * 1e-5).reshape(1, 9), (len(p), 1))


def identity_state(pos=(0.0, 0.0, 0.0), rotvec=None):
    x = np.zeros(36)
    x[:9] = (np.eye(3) if rotvec is None else ob.exp_log(np.asarray(rotvec, float))[0]).reshape(9)
    x[9:12] = pos
    x[21:24] = [0.0, 0.0, -9.81]
    return x


def body_of(x36, pw, P):
    """World points in the body (lidar) frame of a state: body = E^-1 (R^T (p_w - p) - T), float32."""
    R = np.asarray(x36[:9], float).reshape(3, 3)
    p = np.asarray(x36[9:12], float)
    E = np.array(P["extrinsic_R"], float).reshape(3, 3)
    T = np.array(P["extrinsic_T"], float)
    return np.linalg.solve(E, ((np.asarray(pw, float) - p) @ R - T).T).T.astype(np.float32)


def deal_buckets(xyz_body, n_buckets, dt=0.002):
    """Body points -> a time-sorted POINT_DTYPE scan of n_buckets equal runs (curvature = k * dt)."""
    n = len(xyz_body)
    pts = np.zeros(n, dtype=synth.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz_body[:, 0], xyz_body[:, 1], xyz_body[:, 2]
    pts["curvature"] = ((np.arange(n) * n_buckets) // n * dt).astype(np.float32)
    return pts


def layer_counts(cm, max_layer=4):
    """canon_map -> (nodes per layer, planes per layer), layers 0 .. max_layer."""
    nodes, planes = np.zeros(max_layer + 1, int), np.zeros(max_layer + 1, int)

    def walk(n):
        nodes[n["layer"]] += 1
        planes[n["layer"]] += int(n["is_plane"])
        for c in n["children"].values():
            walk(c)

    for n in cm.values():
        walk(n)
    return nodes, planes


def depth(cm):
    def d(n):
        return 1 + max([d(c) for c in n["children"].values()], default=0)

    return max(d(n) for n in cm.values())


def face_lattice(vs=0.4):
    """300 points ON the voxel faces of a 0.4 m grid: (k * 0.4, 0.2, 0.2), k = -50 .. 50 without 0, and the same with the lattice
    coordinate on y and on z (doubles, as that product gives them).  UpdateVoxelMap divides by the FLOAT voxel size
    (voxel_map.cc:337), so its root keys are not floor(p / 0.4)."""
    k = np.array([i for i in range(-50, 51) if i != 0], float) * vs
    out = []
    for ax in range(3):
        p = np.full((len(k), 3), 0.2)
        p[:, ax] = k
        out.append(p)
    p = np.concatenate(out)
    return p, np.tile((np.eye(3) * 1e-4).reshape(1, 9), (len(p), 1))


def naive_keys(p, vs):
    """floor(p / vs) with the DOUBLE voxel size: what the insert must NOT compute."""
    return {tuple(int(v) for v in r) for r in np.floor(np.asarray(p, float) / float(vs)).astype(np.int64)}
