"""-m gpu: lk_downsample_clouds_dev / lk_downsample_clouds - PcdSaver::downsampleAndSave up to the file container, many files per call: contiguous
ranges of registered x y z intensity records in HBM in, one pcl::VoxelGrid-downsampled cloud per range out.

The definition is oracle/preprocess_oracle.py::voxel_grid_centroid with the file's intensity in the place of curvature (restate() below adds
pcl::VoxelGrid's answer to an index overflow: the input unchanged).  Every comparison with it is on bits (uint32 views).  d_world and d_out lie
between devguard's bands in every call: the input comes back unchanged, nothing outside out_off[n_files] records of d_out is written.
"""
import ctypes as C

import numpy as np
import pytest

import devguard
import preprocess_oracle as po
import scenes
import test_overlay_runs as tor
import test_replay_runs as trr
from legkilo_amd import config

pytestmark = pytest.mark.gpu

PT = po.OUT_DTYPE   # x y z curvature: the fourth field carries the intensity here
LEAF = 0.1
SMALL = dict(max_roots=1 << 12, max_nodes=1 << 13, max_point_blocks=1 << 12, max_scan_points=1 << 12)
INVALID = "error -1: "
INT32_MAX = 2147483647


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("LEGKILO_POISON_POOLS", raising=False)
    return monkeypatch


def grid_of(rec, leaf):
    """min_b, div_b and the cell index of every point, in voxel_grid_centroid's own arithmetic."""
    x = np.ascontiguousarray(rec[:, :3], dtype=np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    mn = np.floor(x.min(0) * inv).astype(np.int64)
    div = np.floor(x.max(0) * inv).astype(np.int64) - mn + 1
    ijk = np.floor(x * inv).astype(np.int64) - mn
    return mn, div, ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]


def restate(rec, leaf, reverse=False):
    """One file: float32 [n, 4] -> (float32 [cells, 4], unfiltered).  reverse: the cells' points summed in reverse input order."""
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    _, div, _ = grid_of(rec, leaf)
    if int(div[0]) * int(div[1]) * int(div[2]) > INT32_MAX:
        return rec.copy(), 1
    pts = rec.view(PT).reshape(-1)
    out = po.voxel_grid_centroid(pts[::-1] if reverse else pts, leaf)
    return np.ascontiguousarray(out).view(np.float32).reshape(-1, 4), 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def new_handle(hip_lib):
    return hip_lib.LegKiloHip(config.make_config(None, n_slots=1, **SMALL))


def device_call(g, world, file_off, leaf, name="map clouds"):
    """lk_downsample_clouds_dev between guard bands -> ([file clouds], unfiltered, out_off).  world: float32 [n, 4], ALL of it uploaded (records in front
    of file_off[0] and behind file_off[-1] included)."""
    world = np.ascontiguousarray(world, dtype=np.float32)
    n = int(file_off[-1]) - int(file_off[0])
    gw = devguard.Guarded.input(g, world, offset=16, name=name + " d_world")
    go = devguard.Guarded(g, 16 * n, offset=16, name=name + " d_out")
    try:
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, leaf, go.ptr)
        gw.check()
        got = go.check()
        m = int(out_off[-1])
        assert int(out_off[0]) == 0 and np.all(np.diff(out_off.astype(np.int64)) >= 1) and m <= n
        assert devguard.untouched(got[16 * m:])
        out = np.frombuffer(got[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        return [out[int(a):int(b)] for a, b in zip(out_off[:-1], out_off[1:])], unf, out_off
    finally:
        gw.free()
        go.free()


def check_against_restatement(g, world, file_off, leaf, name):
    clouds, unf, _ = device_call(g, world, file_off, leaf, name)
    assert len(clouds) == len(file_off) - 1 == len(unf)
    flags = []
    for f, got in enumerate(clouds):
        want, u = restate(world[int(file_off[f]):int(file_off[f + 1])], leaf)
        assert same_bits(got, want), (name, f, got.shape, want.shape)
        flags.append(u)
    assert unf.tolist() == flags, name
    return clouds, unf


def base_cloud():
    rng = np.random.default_rng(7)
    rec = np.zeros((1000, 4), dtype=np.float32)
    rec[:, 0] = 100 + rng.uniform(-0.35, 0.35, 1000)
    rec[:, 1] = -50 + rng.uniform(-0.35, 0.35, 1000)
    rec[:, 2] = rng.uniform(-0.15, 0.15, 1000)
    rec[:, 3] = np.where(rng.random(1000) < 0.7, 255.0, 0.0)
    return rec


@pytest.fixture(scope="module")
def base():
    """Test 1's input, shared and left unchanged: the base cloud as the middle file of three, the outer files shifted copies; the restatements."""
    mid = base_cloud()
    world = np.concatenate([mid + np.float32([3.2, -1.6, 0.0, 0.0]), mid, mid + np.float32([-6.4, 0.8, 0.4, 0.0])]).astype(np.float32)
    file_off = np.array([0, 1000, 2000, 3000], dtype=np.uint64)
    fwd, rev = restate(mid, LEAF)[0], restate(mid, LEAF, reverse=True)[0]
    return dict(world=world, file_off=file_off, mid=mid, fwd=fwd, rev=rev, want=[restate(world[a:a + 1000], LEAF)[0] for a in (0, 1000, 2000)])


@pytest.fixture(scope="module")
def handle(hip_lib):
    g = new_handle(hip_lib)
    yield g
    g.close()


def check_base(g, base, name):
    clouds, unf, _ = device_call(g, base["world"], base["file_off"], LEAF, name)
    assert unf.tolist() == [0, 0, 0]
    for f in range(3):
        assert same_bits(clouds[f], base["want"][f]), (name, f)
    return clouds


def test_parity_and_order(handle, base):
    """1. The restatement can see a wrong order on this input (forward and reversed sums differ in 118 of 240 cells); the device gives the forward bits;
    the three files share cell indices and stay three sets of cells."""
    fwd, rev = base["fwd"], base["rev"]
    assert fwd.shape == rev.shape == (240, 4)
    assert int((bits(fwd) != bits(rev)).any(axis=1).sum()) == 118
    assert same_bits(fwd, np.ascontiguousarray(po.voxel_grid_centroid_loops(base["mid"].view(PT).reshape(-1), LEAF)).view(np.float32).reshape(-1, 4))
    idx = [set(grid_of(base["world"][a:a + 1000], LEAF)[2].tolist()) for a in (0, 1000, 2000)]
    assert len(idx[0] & idx[1]) > 100 and len(idx[1] & idx[2]) > 100, "the files share no cell index: a merge across files would not show"
    clouds = check_base(handle, base, "parity")
    assert same_bits(clouds[1], fwd) and not same_bits(clouds[1], rev)
    assert sum(len(c) for c in clouds) == sum(len(i) for i in idx)


def edge_files():
    """Files of 1, 255, 256, 257, 1 and 4 096 points; 300 points in one cell; one cell of 300 points beside 200 cells of one; points on cell faces."""
    rng = np.random.default_rng(4242)

    def cloud(n, centre, half):
        rec = np.zeros((n, 4), dtype=np.float32)
        rec[:, :3] = np.asarray(centre) + rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(half)
        rec[:, 3] = np.where(rng.random(n) < 0.5, 255.0, 0.0)
        return rec

    files = [cloud(1, (2.0, 3.0, -1.0), (0.0, 0.0, 0.0)), cloud(255, (-7.0, 2.0, 0.5), (0.4, 0.4, 0.2)), cloud(256, (5.0, -2.0, 0.0), (0.4, 0.3, 0.2)),
             cloud(257, (-3.0, -3.0, -3.0), (0.5, 0.2, 0.2)), cloud(1, (-0.05, -0.05, -0.05), (0.0, 0.0, 0.0)), cloud(4096, (20.0, -30.0, 1.0), (1.5, 1.5, 0.4))]
    one = cloud(300, (0.35, -0.45, 0.25), (0.04, 0.04, 0.04))                      # a stationary robot: more than a block in one cell
    skew = np.concatenate([cloud(300, (0.35, -0.45, 0.25), (0.04, 0.04, 0.04)), cloud(200, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))])
    skew[300:, 0] = 1.05 + 0.1 * np.arange(200)                                    # 200 cells along x, one point each
    skew = skew[rng.permutation(500)]
    k = np.arange(-3, 4).astype(np.float32) * np.float32(0.1)                      # exactly on cell faces, negative side included: floor, not truncation
    faces = np.zeros((7 ** 3 + 2, 4), dtype=np.float32)
    faces[:343, :3] = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    faces[343, :3] = (-0.0, -0.0, -0.0)
    faces[344, :3] = (-0.0, 0.05, -0.25)
    faces[:, 3] = np.arange(len(faces)) % 3
    assert np.signbit(faces[343, 0])
    files += [one, skew, faces[rng.permutation(len(faces))]]
    assert len(restate(one, LEAF)[0]) == 1 and len(restate(skew, LEAF)[0]) == 201
    return files


@pytest.mark.parametrize("shape", ["mixed", "one_file", "one_point", "files65"])
def test_tile_edges_and_skew(handle, shape):
    """2. Sizes around the 256-point tile, more than a block in one cell, one heavy cell beside many light ones, cell faces, one file (the device-wide
    sort) and 65 files, all behind 13 records that belong to no file."""
    files = edge_files()
    if shape == "one_file":
        files = [files[5]]
    elif shape == "one_point":
        files = [files[0]]
    elif shape == "files65":
        rng = np.random.default_rng(65)
        big = np.concatenate(files)[rng.permutation(sum(len(f) for f in files))]
        cuts = np.r_[0, np.sort(rng.choice(np.arange(1, len(big)), 64, replace=False)), len(big)]
        files = [big[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        assert len(files) == 65
    front = np.full((13, 4), np.float32(np.nan), dtype=np.float32)   # in front of file_off[0]: not read (NaN there would be refused)
    world = np.concatenate([front] + files + [front[:3]])
    file_off = (13 + np.r_[0, np.cumsum([len(f) for f in files])]).astype(np.uint64)
    clouds, unf = check_against_restatement(handle, world, file_off, LEAF, "edges " + shape)
    assert not unf.any()


def test_overflow_fallback(handle):
    """3. div = 1291 per axis is over INT32_MAX cells: that file comes back record for record; its twin with div = 1290 is filtered; -0.0f and the
    input order survive the fallback."""
    twin = np.array([[0, 0, 0, 255], [128.95, 128.95, 128.95, 0]], dtype=np.float32)
    over = np.array([[0, 0, 0, 255], [129.0, 129.0, 129.0, 0]], dtype=np.float32)
    assert grid_of(over, LEAF)[1].tolist() == [1291] * 3 and 1291 ** 3 > INT32_MAX
    assert grid_of(twin, LEAF)[1].tolist() == [1290] * 3 and 1290 ** 3 <= INT32_MAX
    world = np.concatenate([twin, over, twin])
    clouds, unf = check_against_restatement(handle, world, np.array([0, 2, 4, 6], dtype=np.uint64), LEAF, "overflow")
    assert unf.tolist() == [0, 1, 0]
    assert same_bits(clouds[1], over) and len(clouds[0]) == len(clouds[2]) == 2
    # three points of one would-be cell out of index order, a -0.0f, beside a filtered file whose cell they would share
    over2 = np.array([[129.0, 129.0, 129.0, 1], [0.03, 0.02, 0.01, 2], [-0.0, 0.0, 0.0, 3], [0.01, 0.02, 0.03, 4], [64.0, 0.0, 0.0, 5]], dtype=np.float32)
    near = over2[[1, 2, 3]].copy()
    world2 = np.concatenate([near, over2, near])
    clouds2, unf2 = check_against_restatement(handle, world2, np.array([0, 3, 8, 11], dtype=np.uint64), LEAF, "overflow order")
    assert unf2.tolist() == [0, 1, 0] and same_bits(clouds2[1], over2) and len(clouds2[0]) == 1
    assert np.signbit(clouds2[1][2, 0]) and not np.signbit(clouds2[0][0, 0])


def test_refusals(handle, base, hip_lib):
    """4. Every documented refusal with its code, the file named where the contract says so; the bands hold; the handle then passes test 1's call."""
    g = handle
    world, fo = base["world"], base["file_off"]
    n = len(world)
    gw = devguard.Guarded.input(g, world, offset=16, name="refusals d_world")
    go = devguard.Guarded(g, 16 * n, offset=16, name="refusals d_out")

    def refused(match, d_world=None, file_off=fo, leaf=LEAF, d_out=None):
        with pytest.raises(hip_lib.LegKiloError, match=INVALID + ".*" + match):
            g.downsample_clouds_dev(gw.ptr if d_world is None else d_world, file_off, leaf, go.ptr if d_out is None else d_out)

    try:
        refused("n_files is 0", file_off=[0])
        for leaf in (0.0, -0.1, float("nan"), float("inf")):
            refused("leaf", leaf=leaf)
        refused("null", d_world=0)
        refused("null", d_out=0)
        fo_c, oo = np.ascontiguousarray(fo), np.zeros(4, dtype=np.uint64)
        for tabs in ((None, oo.ctypes.data_as(C.c_void_p)), (fo_c.ctypes.data_as(C.c_void_p), None)):   # a null table: past the wrapper
            rc = g.L.lk_downsample_clouds_dev(g.h, C.c_void_p(gw.ptr), C.c_size_t(3), tabs[0], C.c_float(LEAF), C.c_void_p(go.ptr), tabs[1], None)
            assert rc == -1 and b"null" in g.L.lk_last_error(g.h)
        refused("16-byte aligned", d_world=gw.ptr + 4)
        refused("16-byte aligned", d_out=go.ptr + 8)
        refused("overlaps", d_out=gw.ptr + 16 * (n - 1))
        refused("overlaps", d_out=gw.ptr - 16 * (n - 1))
        refused("file_off decreases at file 1", file_off=[0, 1000, 900, 3000])
        refused("file 1 is empty", file_off=[0, 1000, 1000, 3000])
        refused("more than 0x7fffffff points", file_off=[0, 1000, 0x80000000 + 1])
        assert devguard.untouched(go.check())
        gw.check()
        # found on the device, in file 1 of 3
        for bad, what in ((np.nan, "not finite"), (np.inf, "not finite"), (-np.inf, "not finite"), (3e8, "2\\^30"), (-3e8, "2\\^30")):
            w = world.copy()
            w[1000 + 517, 1] = bad
            gw.reset(w)
            refused("file 1 holds a coordinate.*" + what)
            go.check()   # (d_out is undefined behind such an error; the bands are not)
            gw.check()
        w = world.copy()
        w[2999, 3] = np.nan   # the intensity is not a coordinate
        gw.reset(w)
        g.downsample_clouds_dev(gw.ptr, fo, LEAF, go.ptr)
    finally:
        gw.free()
        go.free()
    check_base(g, base, "after refusals")


@pytest.fixture(scope="module")
def scene_plain():
    return scenes.Scene(**tor.CAPS)


@pytest.fixture(scope="module")
def built():
    cases = {}
    yield cases
    for c in cases.values():
        c["g"].close()


def test_from_a_replay(built, oracle_lib, hip_lib, scene_plain):
    """5. d_world_out of lk_batch_replay_runs_cloud_dev, cut into files of two frames, downsampled where it lies: every file is the restatement of the
    host copy of its range; slots, poses and d_world_out are those of a handle that never made the call; map_clouds= gives the same arrays."""
    c = trr.build_case("plain", built, oracle_lib, hip_lib, scene_plain)   # six runs of 3, 1, 4, 2, 1, 3 scans; c["dev"]: the plain entry on its own handle
    runs, tbs, xs = c["runs"], c["tbs"], c["xs"]
    R = len(runs)
    t = hip_lib.flatten_runs(runs, tbs)
    n = len(t["pts"])
    file_off, file_run = hip_lib.pcd_file_offsets(t["run_off"], t["scan_off"], 2)
    assert file_run.tolist() == [0, 0, 1, 2, 2, 3, 4, 5, 5] and int(file_off[0]) == 0 and int(file_off[-1]) == n
    g = trr.new_handle(hip_lib, c["sc"], c["blob"], R)
    d_pts = g.device_malloc(t["pts"].nbytes)
    gw = devguard.Guarded(g, 16 * n, offset=16, name="replay d_world_out")
    go = devguard.Guarded(g, 16 * n, offset=16, name="replay d_out")
    try:
        g.h2d(d_pts, t["pts"])
        g.batch_set_priors(np.asarray(xs), np.asarray([trr.P0] * R))
        poses, _ = g.batch_replay_runs_cloud_dev(d_pts, t["run_off"], t["scan_off"], t["t_begin"], d_world=gw.ptr)
        cloud = gw.read(np.float32).reshape(n, 4).copy()
        assert devguard.sentinel_free(cloud)
        out_off, unf = g.downsample_clouds_dev(gw.ptr, file_off, LEAF, go.ptr)
        assert same_bits(gw.read(np.float32).reshape(n, 4), cloud), "the call changed d_world_out"
        got = go.check()
        m = int(out_off[-1])
        print(f"replay: {n} registered points in {len(file_run)} files -> {m} map points")
        assert devguard.untouched(got[16 * m:]) and 0 < m <= n
        out = np.frombuffer(got[:16 * m].tobytes(), dtype=np.float32).reshape(m, 4)
        clouds = [out[int(a):int(b)] for a, b in zip(out_off[:-1], out_off[1:])]
        for f in range(len(file_run)):
            want, u = restate(cloud[int(file_off[f]):int(file_off[f + 1])], LEAF)
            assert u == unf[f] == 0 and same_bits(clouds[f], want), f
        by_run = [poses[int(a):int(b)] for a, b in zip(t["run_off"][:-1], t["run_off"][1:])]
        X, P = g.batch_get_states(0, R)
        assert trr.same_bits((by_run, X, P, trr.times_of(g, R)), c["dev"]), "the downsampling touched a slot"
        poses2, ex = g.batch_replay_runs(runs, tbs, xs, [trr.P0] * R, cloud=True, map_clouds=(2, LEAF))
        mc = ex["map_clouds"]
        assert tor.pose_bits(poses2) == tor.pose_bits(by_run) and same_bits(ex["cloud"], cloud)
        assert np.array_equal(mc["file_off"], file_off) and np.array_equal(mc["file_run"], file_run) and not mc["unfiltered"].any()
        assert len(mc["clouds"]) == len(clouds) and all(same_bits(a, b) for a, b in zip(mc["clouds"], clouds))
        # the same option on the replay with insert: its own registered cloud, cut and downsampled the same way
        _, exo = g.batch_replay_overlay_runs(runs, tbs, xs, [trr.P0] * R, cloud=True, map_clouds=(2, LEAF))
        mco = exo["map_clouds"]
        assert np.array_equal(mco["file_off"], file_off) and np.array_equal(mco["file_run"], file_run) and len(mco["clouds"]) == len(file_run)
        for f in range(len(file_run)):
            assert same_bits(mco["clouds"][f], restate(exo["cloud"][int(file_off[f]):int(file_off[f + 1])], LEAF)[0]), ("overlay", f)
    finally:
        g.device_free(d_pts)
        gw.free()
        go.free()
        g.close()


def test_host_entry(handle, base):
    """6. lk_downsample_clouds gives the device entry's bits; `out` behind the result keeps what it held."""
    g = handle
    clouds, unf = g.downsample_clouds(base["world"], base["file_off"], LEAF, with_flags=True)
    assert unf.tolist() == [0, 0, 0] and all(same_bits(a, b) for a, b in zip(clouds, base["want"]))
    # a window that starts behind record 0, into a caller's buffer with a pattern in it
    fo = np.array([1000, 2000, 3000], dtype=np.uint64)
    w = np.ascontiguousarray(base["world"])
    out = np.full((2000, 4), np.float32(-7.5), dtype=np.float32)
    out_off = np.zeros(3, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    g._chk(g.L.lk_downsample_clouds(g.h, p(w), C.c_size_t(2), p(fo), C.c_float(LEAF), p(out), p(out_off), None))
    m = int(out_off[-1])
    assert out_off.tolist() == [0, len(base["want"][1]), len(base["want"][1]) + len(base["want"][2])]
    assert same_bits(out[:m], np.concatenate(base["want"][1:])) and np.all(out[m:] == np.float32(-7.5))


def test_poisoned_pools(hip_lib, base, clean_env):
    """7. A fresh handle whose every allocation is filled with 0x5a bytes: the same bits, so no kernel trusts memory nobody wrote."""
    clean_env.setenv("LEGKILO_POISON_POOLS", "1")
    g = new_handle(hip_lib)
    try:
        check_base(g, base, "poisoned")
        assert all(same_bits(a, b) for a, b in zip(g.downsample_clouds(base["world"], base["file_off"], LEAF), base["want"]))
    finally:
        g.close()
