"""The batch residual kernel (lk_residual_kernel, lk_point_kernels.h) issues a lane's scan-point load in its prologue - after the slot / tile
decode and the one word that says which buffer a replay reads, BEFORE the slot's filter state is fetched - and hands the point to residual_tile.
What that order could get wrong, on the smallest shapes that can show it:

* lanes beyond the bucket's end must load nothing: buckets of 1, 63, 64, 65 and 130 points, alone and chained, through lk_batch_replay_dev and
  lk_batch_replay_async_dev, the scan buffer sized exactly between guard bands;
* a point paired with another slot's state: three scans with different points and different priors, first_slot != 0 on the async entry;
* which buffer is read: a shuffled-in-bucket batch as given (lk_batch_order(0)), through lk_batch_prepare_dev's copy, and with the caller's buffer
  overwritten by other scans while the copy exists;
* the XCD-aware launch (LEGKILO_XCDMAP=1; read once per process, so in a child process): 17 tiles in a grid padded to 24 workgroups per scan;
* the other instantiations: rows emitted (lk_batch_residuals_dev) and the hash-table handle (LEGKILO_GRID=0).

Expected values, none of them from the code under test: the oracle's counts (exact) and states (the batch parity tests' tolerance:
rtol 1e-8 / atol 1e-9 on the state, 1e-6 of the largest entry on the covariance), the oracle's rows (1e-9) and valid mask (exact), and equal
bits between two launches that must compute the same thing."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # the XCD test's child process: no conftest has set the paths up
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle")]
    import lk_pkg

    lk_pkg.load()

import scenes
from devguard import Guarded
from legkilo_amd import abi, synth

pytestmark = pytest.mark.gpu

CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
SIZES = (1, 63, 64, 65, 130)
T0 = 1.0
P0 = 1e-4 * np.eye(30)


class Case:
    pass


@pytest.fixture(scope="module")
def case(oracle_lib):
    """One oracle map (first frame, four scans), insert off."""
    c = Case()
    c.sc = scenes.Scene(**CAPS)
    c.o = oracle_lib.Oracle(c.sc.cfg(), imu_mode_only=True)
    c.blob = scenes.mature_oracle_map(c.o, c.sc, T0, n_scans=4)
    c.o.set_map_insert(False)
    yield c
    c.o.close()


def scan_at(c, k, sizes, variant=0, shuffle=False):
    """Scan number k (its own time, points and prior) with buckets of the given sizes, 1 us apart; shuffle: random order inside every bucket."""
    tb = T0 + 0.6 + 0.13 * k
    n = int(sum(sizes))
    sc = synth.dense_scan(c.sc.world, scenes.Frozen(c.sc.traj, tb), tb, c.sc.P, n=n, n_buckets=1, seed_scan=4100 + k + 1000 * variant,
                          seed_noise=5200 + k + 1000 * variant)
    assert len(sc) == n
    sc["curvature"] = np.repeat(np.arange(len(sizes), dtype=np.float32) * np.float32(1e-6), sizes)
    if shuffle:
        rng = np.random.default_rng([77, k, variant])
        e = np.cumsum(sizes)
        for a, b in zip(e - np.array(sizes), e):
            sc[a:b] = sc[a:b][rng.permutation(b - a)]
    off, dt = synth.buckets_of(sc)
    assert np.array_equal(np.diff(off.astype(np.int64)), sizes)
    x = synth.initial_state(c.sc.traj, tb, c.sc.P, np.random.default_rng([6160, k]), 0.02, 0.5)
    return sc, x, off, dt


def oracle_scan(c, scan, x):
    o = c.o
    o.set_state(x, P0)
    o.set_times(0.0, 0.0)
    po, _ = o.process_scan(scan, 0.0)
    xo, Po = o.get_state()
    return (int(po.n_buckets), int(po.n_updates), int(po.n_effect)), xo.copy(), Po.copy()


def handle(hip_lib, c, n_slots, monkeypatch=None, grid=True):
    if not grid:
        monkeypatch.setenv("LEGKILO_GRID", "0")
    try:
        g = hip_lib.LegKiloHip(c.sc.cfg(n_slots=n_slots))
    finally:
        if not grid:
            monkeypatch.delenv("LEGKILO_GRID")
    g.map_import(c.blob)
    g.init_process_cov_q()
    return g


_PINNED = []


def pinned_poses(n):
    import torch

    t = torch.zeros(n * abi.pose_dtype().itemsize, dtype=torch.uint8).pin_memory()
    _PINNED.append(t)
    return t.numpy().view(abi.pose_dtype())


def counts(pose):
    return int(pose["n_buckets"]), int(pose["n_updates"]), int(pose["n_effect"])


def replay_sync(g, d_pts, xs, n_pts, off, dt):
    """lk_batch_replay_dev on slots [0, S): per slot (counts, x36, P)."""
    S = len(xs)
    g.batch_set_priors(np.array(xs), np.array([P0] * S))
    poses = np.frombuffer(g.batch_replay_dev(d_pts, S, n_pts, 0.0, off, dt), dtype=abi.pose_dtype()).copy()
    X, P = g.batch_get_states(0, S)
    return [(counts(poses[s]), X[s].copy(), P[s].copy()) for s in range(S)]


def replay_async(g, d_pts, first_slot, xs, n_pts, off, dt):
    """lk_batch_replay_async_dev on slots [first_slot, first_slot + S) with the priors in HBM: per slot (counts, x36, P)."""
    S = len(xs)
    x = np.ascontiguousarray(np.array(xs))
    P = np.ascontiguousarray(np.array([P0] * S).reshape(S, 900))
    d_x, d_P = g.device_malloc(x.nbytes), g.device_malloc(P.nbytes)
    g.h2d(d_x, x)
    g.h2d(d_P, P)
    out = pinned_poses(S)
    g.batch_replay_async_dev(d_pts, first_slot, S, n_pts, 0.0, off, dt, d_x36=d_x, d_P900=d_P, host_out_ptr=out.ctypes.data)
    g.synchronize()
    X, Pg = g.batch_get_states(first_slot, S)
    for d in (d_x, d_P):
        g.device_free(d)
    return [(counts(out[s]), X[s].copy(), Pg[s].copy()) for s in range(S)]


def check_against_oracle(tag, got, want):
    (cnt_g, xg, Pg), (cnt_o, xo, Po) = got, want
    assert cnt_g == cnt_o, (tag, cnt_g, cnt_o)
    assert np.allclose(xo, xg, rtol=1e-8, atol=1e-9), (tag, np.abs(xo - xg).max())
    assert np.abs(Pg - Po).max() <= 1e-6 * np.abs(Po).max(), (tag, np.abs(Pg - Po).max() / np.abs(Po).max())


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ----------------------------------------------------------------------------- lanes beyond the bucket's end
def test_lanes_beyond_the_buckets_end(case, hip_lib):
    """One bucket of 1, 63, 64, 65, 130 points, then the five as one scan of five buckets; two slots (the same points under two priors), the
    buffer exactly 2 x n points between guard bands.  Both entries; the async one on slots [2, 4)."""
    c = case
    g = handle(hip_lib, c, 4)
    total = 0
    for k, sizes in enumerate([(n,) for n in SIZES] + [SIZES]):
        scan, xa, off, dt = scan_at(c, k, sizes)
        xb = synth.initial_state(c.sc.traj, T0 + 0.6 + 0.13 * k, c.sc.P, np.random.default_rng([7170, k]), 0.02, 0.5)
        want = [oracle_scan(c, scan, x) for x in (xa, xb)]
        assert want[0][0][0] == len(sizes)
        total += want[0][0][2] + want[1][0][2]
        gp = Guarded.input(g, np.concatenate([scan, scan]), offset=16, name=f"prologue d_pts {k}")
        got_s = replay_sync(g, gp.ptr, [xa, xb], len(scan), off, dt)
        got_a = replay_async(g, gp.ptr, 2, [xa, xb], len(scan), off, dt)
        gp.check()
        gp.free()
        for s in range(2):
            print("sizes", sizes, "slot", s, "oracle", want[s][0], "sync", got_s[s][0], "async", got_a[s][0])
            check_against_oracle(("sync", sizes, s), got_s[s], want[s])
            check_against_oracle(("async", sizes, s), got_a[s], want[s])
            assert same_bits(got_s[s], got_a[s]), (sizes, s)
    assert total > 0
    g.close()


# ----------------------------------------------------------------------------- point and state of the same slot
def test_point_and_state_of_the_same_slot(case, hip_lib):
    """Three scans, each with its own points and its own prior: a point read from one slot's scan and transformed by another slot's pose gives
    another scan's matches.  Precondition, on the oracle alone: scan s under prior s +- 1 does NOT give scan s's result."""
    c = case
    sizes = (100, 93)
    parts = [scan_at(c, 10 + s, sizes) for s in range(3)]
    off, dt = parts[0][2], parts[0][3]
    xs = [p[1] for p in parts]
    want = [oracle_scan(c, p[0], p[1]) for p in parts]
    for s in range(3):
        assert want[s][0][1] == len(sizes) and want[s][0][2] > 0, want[s][0]
        wrong = oracle_scan(c, parts[s][0], xs[(s + 1) % 3])
        assert wrong[0] != want[s][0] or not np.allclose(wrong[1], want[s][1], rtol=1e-8, atol=1e-9), s
    g = handle(hip_lib, c, 9)
    n = int(sum(sizes))
    gp = Guarded.input(g, np.concatenate([p[0] for p in parts]), offset=16, name="prologue three scans")
    got_s = replay_sync(g, gp.ptr, xs, n, off, dt)
    got_a = replay_async(g, gp.ptr, 3, xs, n, off, dt)   # (the entry wants first_slot a multiple of n_scans)
    gp.check()
    gp.free()
    for s in range(3):
        print("slot", s, "oracle", want[s][0], "sync", got_s[s][0], "async (first_slot 3)", got_a[s][0])
        check_against_oracle(("sync", s), got_s[s], want[s])
        check_against_oracle(("async", s), got_a[s], want[s])
        assert same_bits(got_s[s], got_a[s]), s
    g.close()


# ----------------------------------------------------------------------------- which buffer is read
def test_which_buffer_is_read(case, hip_lib):
    """S = 3 scans of 2 048 points in 4 buckets of 512, random order inside every bucket (6 144 points: above the 4 096 a batch needs to be
    tracked).  As given; through lk_batch_prepare_dev's voxel-ordered copy; and with the caller's buffer overwritten by three other scans while
    the copy exists - each against the oracle on the scans the buffer holds at that replay."""
    c = case
    sizes = (512,) * 4
    A = [scan_at(c, 20 + s, sizes, shuffle=True) for s in range(3)]
    B = [scan_at(c, 30 + s, sizes, shuffle=True) for s in range(3)]
    off, dt = A[0][2], A[0][3]
    want = {name: [oracle_scan(c, p[0], p[1]) for p in parts] for name, parts in (("A", A), ("B", B))}
    for s in range(3):
        assert want["A"][s][0][1] >= 3 and want["B"][s][0][1] >= 3 and want["A"][s][0][2] > 400 and want["B"][s][0][2] > 400
        assert np.abs(want["A"][s][1][9:12] - want["B"][s][1][9:12]).max() > 1e-4, s   # the wrong content does not pass the tolerance
    g = handle(hip_lib, c, 3)
    ptsA, ptsB = np.concatenate([p[0] for p in A]), np.concatenate([p[0] for p in B])
    xA, xB = [p[1] for p in A], [p[1] for p in B]
    d_pts = g.device_malloc(ptsA.nbytes)
    g.h2d(d_pts, ptsA)
    g.batch_order(0)
    given = replay_sync(g, d_pts, xA, 2048, off, dt)
    g.batch_order(1)
    g.batch_set_priors(np.array(xA), np.array([P0] * 3))
    g.batch_prepare_dev(d_pts, 3, 2048, off)
    assert g.batch_order_stats() == (1, 1, 0), g.batch_order_stats()
    copied = replay_sync(g, d_pts, xA, 2048, off, dt)
    g.h2d(d_pts, ptsB)                        # other scans where the copy was made from
    over = replay_sync(g, d_pts, xB, 2048, off, dt)
    g.batch_order(0)
    givenB = replay_sync(g, d_pts, xB, 2048, off, dt)
    for s in range(3):
        print("slot", s, "oracle A", want["A"][s][0], "given", given[s][0], "copy", copied[s][0], "| oracle B", want["B"][s][0], "overwritten", over[s][0])
        check_against_oracle(("given", s), given[s], want["A"][s])
        check_against_oracle(("copy", s), copied[s], want["A"][s])
        check_against_oracle(("overwritten", s), over[s], want["B"][s])
        assert same_bits(over[s], givenB[s]), s          # the caller's buffer, in the caller's order
    assert not all(same_bits(given[s], copied[s]) for s in range(3))   # another order of the same points: the copy WAS read
    g.device_free(d_pts)
    g.close()


# ----------------------------------------------------------------------------- XCD-aware launch
def xcd_child(path_in, path_out):
    """Child process of test_xcd_aware_launch: one replay of the batch in path_in, results to path_out."""
    import torch  # noqa: F401  (binding.lib() brings torch's HIP runtime up first, as the hip_lib fixture does)
    from legkilo_amd import binding

    d = np.load(path_in)
    S, n_pts = int(d["S"]), int(d["n_pts"])
    g = binding.LegKiloHip(scenes.Scene(**CAPS).cfg(n_slots=S))
    g.map_import(d["blob"])
    g.init_process_cov_q()
    d_pts = g.device_malloc(d["pts"].nbytes)
    g.h2d(d_pts, d["pts"])
    g.batch_set_priors(d["x"], np.array([P0] * S))
    poses = np.frombuffer(g.batch_replay_dev(d_pts, S, n_pts, 0.0, d["off"], d["dt"]), dtype=abi.pose_dtype()).copy()
    X, P = g.batch_get_states(0, S)
    g.device_free(d_pts)
    g.close()
    np.savez(path_out, cnt=np.array([counts(poses[s]) for s in range(S)]), X=X, P=P)


def test_xcd_aware_launch(case, tmp_path):
    """Two scans, one bucket of 1 025 points: 17 tiles, the XCD-aware grid has 8 x ceil(17 / 8) = 24 workgroups per scan, seven of which leave
    before any load.  LEGKILO_XCDMAP is read once per process: one child with it, one without - the same bits, and the oracle's result."""
    c = case
    parts = [scan_at(c, 40 + s, (1025,)) for s in range(2)]
    want = [oracle_scan(c, p[0], p[1]) for p in parts]
    assert all(w[0][2] > 0 for w in want)
    path_in = tmp_path / "in.npz"
    np.savez(path_in, blob=np.asarray(c.blob, dtype=np.uint8), pts=np.concatenate([p[0] for p in parts]), x=np.array([p[1] for p in parts]), off=parts[0][2],
             dt=parts[0][3], S=2, n_pts=1025)
    res = {}
    for name, val in (("xcd", "1"), ("plain", "0")):
        env = dict(os.environ, LEGKILO_XCDMAP=val)
        path_out = tmp_path / f"{name}.npz"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(path_in), str(path_out)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
        d = np.load(path_out)
        res[name] = [(tuple(int(v) for v in d["cnt"][s]), d["X"][s], d["P"][s]) for s in range(2)]
    for s in range(2):
        print("slot", s, "oracle", want[s][0], "xcd", res["xcd"][s][0], "plain", res["plain"][s][0])
        check_against_oracle(("xcd", s), res["xcd"][s], want[s])
        assert same_bits(res["xcd"][s], res["plain"][s]), s


# ----------------------------------------------------------------------------- the other instantiations
def test_rows_emitted_and_hash_table_handle(case, hip_lib, monkeypatch):
    """lk_batch_residuals_dev (lk_residual_kernel<true, ...>) on scans of 1, 63, 64, 65, 130 points and on the chained one, two slots under two
    states: rows to 1e-9, valid mask exact, output buffers between guard bands; and the same calls - rows and replay - on a LEGKILO_GRID=0 handle
    (the hash-table instantiations): bit for bit the grid handle."""
    c = case
    gg, gh = handle(hip_lib, c, 2), handle(hip_lib, c, 2, monkeypatch, grid=False)
    n_valid = 0
    for k, sizes in enumerate([(n,) for n in SIZES] + [SIZES]):
        scan, xa, off, dt = scan_at(c, k, sizes)
        xb = synth.initial_state(c.sc.traj, T0 + 0.6 + 0.13 * k, c.sc.P, np.random.default_rng([7170, k]), 0.02, 0.5)
        n = len(scan)
        both = np.concatenate([scan, scan])
        got = {}
        for name, g in (("grid", gg), ("pool", gh)):
            gp = Guarded.input(g, both, offset=16, name=f"rows d_pts {k}")
            g_rows = Guarded(g, 2 * n * 64, offset=16, name=f"rows d_rows8 {k}")
            g_v = Guarded(g, 2 * n, offset=1, name=f"rows d_valid {k}")
            g.batch_set_priors(np.array([xa, xb]), np.array([P0, P0]))
            g.batch_residuals_dev(gp.ptr, 2, n, g_rows.ptr, g_v.ptr)
            g.synchronize()
            rows8 = g_rows.read(np.float64).reshape(2 * n, 8).copy()
            v = g_v.read(np.uint8).copy()
            rep = replay_sync(g, gp.ptr, [xa, xb], n, off, dt)
            gp.check()
            for q in (gp, g_rows, g_v):
                q.free()
            got[name] = (rows8, v, rep)
        rows8, v, rep = got["grid"]
        assert np.array_equal(got["pool"][0], rows8) and np.array_equal(got["pool"][1], v), sizes
        for s in range(2):
            assert same_bits(got["pool"][2][s], rep[s]), (sizes, s)
        xyz = scenes.xyz_of(scan)
        for s, x in enumerate((xa, xb)):
            c.o.set_state(x, P0)
            ho, zo, Ro, vo = c.o.residuals(xyz)
            a, b = s * n, (s + 1) * n
            assert np.array_equal(vo.astype(np.uint8), v[a:b]), (sizes, s, np.flatnonzero(vo.astype(np.uint8) != v[a:b]))
            n_valid += int(vo.sum())
            scenes.rows_close(np.ascontiguousarray(rows8[a:b, :6]), rows8[a:b, 6], rows8[a:b, 7], ho, zo, Ro, v[a:b], rtol=1e-9)
    assert n_valid > 0
    gg.close()
    gh.close()


if __name__ == "__main__":
    xcd_child(sys.argv[1], sys.argv[2])
