"""The range gate of the frozen-map grid (records carry lk_range_bound(radius), two float compares) against the gate of the pool records
(sqrtf, LEGKILO_GRID=0) on points laid ACROSS the gate: for eight planes of an oracle map, 512 points in the plane whose distance from the
plane's centre steps by 8e-8 (relative) through 3 * radius * (1 -+ 2e-5) - float spacing of the gated quantity on both sides of its
threshold.  Both paths must accept exactly the points the oracle accepts, and leave the same bits in the filter.

`origin` is the room as legkilo_amd.synth builds it; `negz` and `far` move room and trajectory (tests/placement.py): the gate's
(float)(p - c) is formed from coordinates of 10 m and of 3 km, where a kernel that subtracted two floats would be wrong by metres."""
import numpy as np
import pytest

import placement
import scenes
from legkilo_amd import abi, synth

pytestmark = pytest.mark.gpu

CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
N_PLANES, PER_PLANE = 8, 512     # four root planes + four planes of the grid's flattened lists: the oracle splits eight ladders at every placement
STEP, HALF = 8e-8, PER_PLANE // 2   # 256 * 8e-8 = 2.05e-5 on either side


def ladder(c, e, radius):
    """World points c + t e, t across 3 * radius (radius: the plane's float)."""
    t = 3.0 * float(radius) * (1.0 + (np.arange(PER_PLANE) - HALF) * STEP)
    return c[None, :] + t[:, None] * e[None, :]


def body_of(x36, pw, P):
    R, p = x36[:9].reshape(3, 3), x36[9:12]
    E = np.array(P["extrinsic_R"], float).reshape(3, 3)
    T = np.array(P["extrinsic_T"], float)
    return (((pw - p) @ R - T) @ E).astype(np.float32)


def plane_candidates(blob, vs):
    """(radius, root key, centre, in-plane direction, the root itself is the plane) of planes whose gate lies INSIDE their root voxel along that direction, so that the ladder's
    points look the plane's own root up; widest planes first."""
    b = abi.parse_blob(blob)
    nodes, planes = b["nodes"], b["planes"]
    out = []
    for r in b["roots"]:
        lo = np.array(r["key"], float) * vs
        stack = [int(r["node"])]
        while stack:
            i = stack.pop()
            if planes[i]["flags"] & abi.LK_PLANE_IS_PLANE:
                pl = planes[i]
                c, n, T = np.array(pl["center"], float), np.array(pl["normal"], float), 3.0 * float(pl["radius"])
                u = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
                u /= np.linalg.norm(u)
                v = np.cross(n, u)
                for a in np.arange(16) * (np.pi / 8):
                    e = np.cos(a) * u + np.sin(a) * v
                    far = c + 1.001 * T * e
                    if np.all(far > lo + 0.01) and np.all(far < lo + vs - 0.01):
                        out.append((float(pl["radius"]), tuple(int(k) for k in r["key"]), c, e, i == int(r["node"])))
                        break
                continue
            stack += [int(k) for k in nodes[i]["child"] if k >= 0]
    out.sort(key=lambda q: -q[0])
    return out


def ladder_case(oracle_lib, place):
    """The oracle's side: scene, map blob, prior, the scan of N_PLANES ladders, its bucket table and the oracle's replay of it ->
    (sc, blob, x0, P0, scan, off, dt, valid [N_PLANES, PER_PLANE], oracle pose)."""
    sc = scenes.Scene(**CAPS) if place == "origin" else placement.placed_scene(place, **CAPS)
    D = np.array(placement.PLACEMENTS[place])
    o = oracle_lib.Oracle(sc.cfg(), imu_mode_only=True)
    t0 = 1.0
    scenes.mature_oracle_map(o, sc, t0, n_scans=4)
    # clutter (corner clusters of 0.25 m cells): cut voxels, so that some ladders run through the grid's flattened lists
    centre = sc.traj.pos(t0 + 1.3)
    # (moved with the room by D snapped to whole voxels: the clutter cuts the same voxels, relative to the grid, at every placement)
    vs = float(sc.P["voxel_size"])
    snap = np.round(D / vs) * vs - D
    clutter = scenes.corner_clutter(np.random.default_rng(77), n_cells=40, per_cell=80,
                                    origin=(centre[0] + 2.0 + snap[0], centre[1] - 1.0 + snap[1], 3.0 + D[2] + snap[2]))
    o.map_update(clutter, np.tile((1e-4 * np.eye(3)).reshape(1, 9), (len(clutter), 1)))
    blob = o.map_export()
    o.set_map_insert(False)
    x0 = synth.initial_state(sc.traj, t0 + 1.3, sc.P)
    P0 = 1e-4 * np.eye(30)
    o.set_state(x0, P0)
    # eight planes whose ladder the ORACLE's gate splits (a ladder no other candidate of the voxel, nor the neighbour retry, fills in): four root
    # planes (the grid cell's own record) and four planes below a cut root (records of the grid's flattened lists)
    chosen, used, room = [], set(), {True: N_PLANES // 2, False: N_PLANES // 2}
    for radius, key, c, e, at_root in plane_candidates(blob, float(sc.P["voxel_size"])):
        if key in used or room[at_root] == 0:
            continue
        xb = body_of(x0, ladder(c, e, np.float32(radius)), sc.P)
        v = o.residuals(xb)[3]
        if 0 < int(v.sum()) < PER_PLANE:
            chosen.append(xb)
            used.add(key)
            room[at_root] -= 1
            if len(chosen) == N_PLANES:
                break
    assert len(chosen) == N_PLANES, len(chosen)
    xb = np.concatenate(chosen)
    valid = o.residuals(xb)[3].reshape(N_PLANES, PER_PLANE)
    for k in range(N_PLANES):   # the ladder really straddles the gate
        assert 0 < int(valid[k].sum()) < PER_PLANE, (k, int(valid[k].sum()))
    scan = np.zeros(len(xb), dtype=synth.POINT_DTYPE)
    scan["x"], scan["y"], scan["z"] = xb[:, 0], xb[:, 1], xb[:, 2]
    off, dt = synth.buckets_of(scan)
    assert len(dt) == 1
    o.set_state(x0, P0)
    o.set_times(0.0, 0.0)
    po, _ = o.process_scan(scan, 0.0)
    assert po.n_effect == int(valid.sum())
    print(place, "accepted per plane:", valid.sum(1).tolist(), "of", PER_PLANE)
    o.close()
    return sc, blob, x0, P0, scan, off, dt, valid, po


@pytest.mark.parametrize("place", ["origin", "negz", "far"])
def test_range_gate_ladder_grid_equals_pool_records(oracle_lib, hip_lib, monkeypatch, place):
    sc, blob, x0, P0, scan, off, dt, valid, po = ladder_case(oracle_lib, place)
    res = {}
    for name, env in (("grid", {}), ("pool", {"LEGKILO_GRID": "0"})):
        monkeypatch.delenv("LEGKILO_GRID", raising=False)
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        g = hip_lib.LegKiloHip(sc.cfg(n_slots=1))
        g.map_import(blob)
        g.init_process_cov_q()
        d_pts = g.device_malloc(scan.nbytes)
        g.h2d(d_pts, scan)
        g.batch_set_priors(x0[None], P0[None])
        poses = g.batch_replay_dev(d_pts, 1, len(scan), 0.0, off, dt)
        X, P = g.batch_get_states(0, 1)
        res[name] = (int(poses[0].n_effect), int(poses[0].n_updates), X.copy(), P.copy())
        g.device_free(d_pts)
        g.close()
    monkeypatch.delenv("LEGKILO_GRID", raising=False)
    print("n_effect grid", res["grid"][0], "pool", res["pool"][0], "oracle", po.n_effect)
    assert res["grid"][0] == res["pool"][0] == po.n_effect
    assert res["grid"][1] == res["pool"][1] == po.n_updates
    assert np.array_equal(res["grid"][2], res["pool"][2]) and np.array_equal(res["grid"][3], res["pool"][3])
