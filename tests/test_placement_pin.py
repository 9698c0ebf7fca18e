"""Pins the oracle against the reference's own KILO::process AWAY from the origin (tests/placement.py): what makes it a checker at
the placements of tests/test_placement.py, as tests/test_reference_pin.py does for tests/offconfig.py.

What holds at every placement, and is asserted: the first-frame map bit for bit; the first two scans (match counts equal, states to
1e-12 ABSOLUTE - an rtol would allow 3e-5 m on a position of 3 km); match counts of four scans; every plane of both maps within
the rounding bound B of placement.plane_fit_errors.  What does not hold, and is therefore not asserted: closed-loop state
agreement after the map has been refitted from inserted points - see test_four_scans_counts_and_plane_fits.
"""
import numpy as np
import pytest

import oracle_binding as ob
import placement
import scenes

pytestmark = pytest.mark.skipif(ob.build_ref() is None, reason="oracle/_ref not built and the reference's sources absent")

PLACES = ("negz", "neg", "far")
N_SCANS = 4
_runs = {}


def run(place, use_kin, tmp_path_factory):
    """Oracle and reference through the first frame and N_SCANS config-1 scans at a placement, once per module run ->
    dict(first=(blob_o, blob_k), scans=[(pose_o, x_o, pose_k, x_k)], maps=(blob_o, blob_k))."""
    key = (place, use_kin)
    if key not in _runs:
        sc = placement.placed_scene(place, None, use_kin)
        o = ob.Oracle(sc.cfg(), imu_mode_only=not use_kin)
        k = ob.ReferenceKilo(sc.P, not use_kin, tmp_path_factory.mktemp("ref") / "ref.yaml")
        t0 = 1.0
        for obj in (o, k):
            x0 = scenes.init_filter(obj, sc, t0)
            scenes.first_frame(obj, sc, t0, x0)
        first = (bytes(o.map_export()), bytes(k.map_export()))
        ro = scenes.replay_vlp(o, sc, t0, N_SCANS, use_kin=use_kin)
        rk = scenes.replay_vlp(k, sc, t0, N_SCANS, use_kin=use_kin)
        _runs[key] = dict(first=first, scans=[(po, xo, pk, xk) for (po, xo), (pk, xk) in zip(ro, rk)],
                          maps=(bytes(o.map_export()), bytes(k.map_export())))
        o.close()
        k.close()
    return _runs[key]


def u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def maps_identical_up_to_the_eigen_solver(blob_a, blob_b):
    """scenes.maps_identical, except that a plane's normal may differ by 4 ulp of 1.0 (4.5e-16, up to sign) and its plane_var by 4e-15 of
    its largest entry: oracle and reference solve the 3 x 3 symmetric eigenproblem with different Jacobi-type stand-ins for Eigen's
    EigenSolver (tests/test_reference_pin.py, test_init_plane), whose eigenvectors agree to the last bits only.  Everything else -
    voxels, tree shape, counters, state bits, stored points, centre, d, radius, eigenvalues (floats) - bit for bit.
    -> (roots, planes, planes whose normal or plane_var differ at all, largest normal difference, largest relative plane_var difference)."""
    A, B = scenes.canon_map(blob_a), scenes.canon_map(blob_b)
    assert set(A) == set(B), ("root key sets differ", len(A), len(B))
    st = dict(roots=len(A), planes=0, differ=0, normal=0.0, plane_var=0.0)

    def same(a, b, where):
        for f in ("layer", "npts", "new_points", "is_plane", "state", "quater"):
            assert a[f] == b[f], (where, f, a[f], b[f])
        assert np.array_equal(a["center"], b["center"]), (where, "center")
        if a["is_plane"]:
            st["planes"] += 1
            for f in ("center", "d", "radius", "flags", "points_size", "min_ev", "mid_ev", "max_ev"):
                assert np.array_equal(a["plane"][f], b["plane"][f]), (where, "plane", f)
            na, nb = a["plane"]["normal"], b["plane"]["normal"]
            va, vb = scenes._expand21(a["plane"]["plane_var"]), scenes._expand21(b["plane"]["plane_var"])
            if np.dot(na, nb) < 0:
                nb = -nb
                vb[:3, 3:] *= -1.0
                vb[3:, :3] *= -1.0
            dn, dv = float(np.abs(na - nb).max()), float(np.abs(va - vb).max() / np.abs(va).max())
            st["differ"] += int(dn > 0 or dv > 0)
            st["normal"], st["plane_var"] = max(st["normal"], dn), max(st["plane_var"], dv)
            assert dn <= 4 * 2.0 ** -52 and dv <= 4e-15, (where, dn, dv)
        assert (a["pts"] is None) == (b["pts"] is None), (where, "points presence")
        if a["pts"] is not None:
            assert np.array_equal(a["pts"]["pw"], b["pts"]["pw"]) and np.array_equal(a["pts"]["var"], b["pts"]["var"]), (where, "points")
        assert set(a["children"]) == set(b["children"]), (where, "children")
        for o in a["children"]:
            same(a["children"][o], b["children"][o], where + (o,))

    for k in A:
        same(A[k], B[k], (k,))
    return st


@pytest.mark.parametrize("use_kin", [False, True])
@pytest.mark.parametrize("place", PLACES)
def test_first_frame_maps_are_identical(tmp_path_factory, place, use_kin):
    """BuildVoxelMap of the first VLP-16 frame at the placement: same voxels, tree shape, counters, stored points and plane records bit
    for bit - except the eigenvector-derived fields of a few dozen planes, which differ in the last bits AT EVERY placement, the origin
    included (origin: 37 of ~2 500 planes, normal 8e-17, plane_var 2.4e-16 relative; far: 52 planes, 1.4e-17, 3.9e-16).  Plain
    scenes.maps_identical therefore fails between these two builds, here as at the origin; the placement adds nothing to it."""
    r = run(place, use_kin, tmp_path_factory)
    st = maps_identical_up_to_the_eigen_solver(u8(r["first"][0]), u8(r["first"][1]))
    print(f"{place} use_kin={use_kin}: {st}")
    assert st["roots"] > 500 and st["planes"] > 500 and st["differ"] < st["planes"] // 20, st


@pytest.mark.parametrize("use_kin", [False, True])
@pytest.mark.parametrize("place", PLACES)
def test_scans_0_and_1_states_to_1e12_absolute(tmp_path_factory, place, use_kin):
    """Scans 0 and 1 through KILO::process on the (identical) first-frame map: n_effect equal and above 300, every state component
    within 1e-12 absolute.  Measured maxima over both scans (negz / neg / far) - IMU-only: 2.7e-15 / 5.6e-17 / 3.3e-16; leg fusion:
    5.2e-18 / 5.6e-17 / 5.6e-17.  Both scans still match planes of the first frame (inserted points refit a plane only once enough
    of them have gathered), so the sides differ by re-association only; the margin to 1e-12 is for that not to become a flaky bar."""
    r = run(place, use_kin, tmp_path_factory)
    worst = 0.0
    for s in (0, 1):
        po, xo, pk, xk = r["scans"][s]
        assert po.n_effect == pk.n_effect > 300, (s, po.n_effect, pk.n_effect)
        worst = max(worst, float(np.abs(xo - xk).max()))
    print(f"{place} use_kin={use_kin}: max |x_oracle - x_reference| over scans 0-1 = {worst:.2e}")
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("use_kin", [False, True])
@pytest.mark.parametrize("place", PLACES)
def test_four_scans_counts_and_plane_fits(tmp_path_factory, place, use_kin):
    """Four scans, closed loop: match counts equal scan by scan, and every plane of BOTH maps within 1.0 x B (normal) and 1e-9 m
    (centre) of the long-double fit of its own stored points, at least 2 000 planes per map.

    No assertion on closed-loop state agreement.  With the world and trajectory moved by D (config 1, IMU-only):

      D (m)                        first-frame map   states, scans 0-1   states, scan 3   planes after 4 scans (normal / d)
      (0, 0, 0)                    bit-equal         <= 3e-12            3e-9             2e-8 / 2e-6
      (-100.3, -80.7, -40.2)       bit-equal         <= 6e-17            3e-7             1.4e-4 / 4e-3
      (3000.25, -2000.4, -150.1)   bit-equal         <= 3.3e-16          1.9e-5           9e-4 / 2 m; one root key differs
      (600000.3, 70.2, -30.1)      -                 1.6e-4 (scan 0)     counts differ from scan 1

    The divergence comes from plane refits after inserts: the raw-moment covariance carries an absolute error of about eps |p|^2, and
    the reference stores plane d as float.  A tight closed-loop tolerance is no property of the reference away from the origin; the
    per-scan differences are printed so that they stay in the logs.  Measured here, largest |dx| after scan 3 (negz / neg / far):
    IMU-only 1.3e-8 / 3.2e-7 / 1.9e-5, leg fusion 6.2e-13 / 9.5e-8 / 8.8e-7.  Largest normal error / B over both modes: oracle
    0.180 / 0.205 / 0.186, reference 0.173 / 0.191 / 0.172 (p99 <= 0.10; 2 537 .. 2 698 planes each); largest centre error
    8.9e-15 / 3.9e-14 / 1.2e-12 m."""
    r = run(place, use_kin, tmp_path_factory)
    for s, (po, xo, pk, xk) in enumerate(r["scans"]):
        print(f"{place} use_kin={use_kin} scan {s}: n_effect {int(po.n_effect)} / {int(pk.n_effect)}, max |dx| {np.abs(xo - xk).max():.2e}")
        assert po.n_effect == pk.n_effect, (s, po.n_effect, pk.n_effect)     # (the reference's pose carries no bucket / update counts)
    for side, blob in zip(("oracle", "reference"), r["maps"]):
        en, ec, B = placement.plane_fit_errors(u8(blob))
        print(f"{place} use_kin={use_kin} {side}: {len(en)} planes, max normal error / B {np.max(en / B):.3f} (p99 {np.quantile(en / B, 0.99):.3f}), "
              f"max centre error {ec.max():.2e} m")
        assert len(en) >= 2000, (side, len(en))
        assert (en <= 1.0 * B).all(), (side, float(np.max(en / B)))
        assert ec.max() <= 1e-9, (side, float(ec.max()))
