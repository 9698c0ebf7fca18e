"""lk_batch_order (default LK_BATCH_ORDER_AUTO) on the entry it was built for: lk_batch_replay_async_dev, which never synchronises.  Which memory a replay's
residual launches read - the caller's batch or the library's voxel-ordered copy of it - is decided by a state machine split between the host (which picks
the stamp kernel's mode from a host-mapped count that lags behind the replays in flight) and the device (lk_batch_stamp.h; the decision alone is enumerated
on the CPU in tests/test_batch_stamp.py).  Here the whole of it runs on the GPU: copy made and read on all three ring streams, new content in a sorted batch's
buffer with TWO replays enqueued before the device has looked at either (on one stream, and across two), content that goes back, more buffers than cache
entries, the edit the sample cannot see, the tracking threshold, lk_batch_prepare_dev in LK_BATCH_ORDER_AS_GIVEN.

Shapes: S = 3 scans of 2 048 points (4 buckets of 512, random order inside every bucket) per slot range, n_slots = 9: three ring streams; 6 144 points, so
the stamp samples points 0 .. 4 095 (stride 1) and all of scan 2 lies outside the sample.  The reference is the oracle's process_scan per slot with the map
insert off (counts exact, state rtol 1e-8 / atol 1e-9, as test_batch_sort_by_voxel); replays of the same points in the same order must agree bit for bit:
with the batch as given under LK_BATCH_ORDER_AS_GIVEN, or with the synchronous replay of lk_batch_sort_by_voxel_dev's output under the same priors.

The two replays that race the device (T2, T3) sit behind a bounded filler (torch.cuda._sleep on the handle's stream) sized in the test to 20 x the measured
host time of two enqueues; that the filler had not finished when the second enqueue returned is asserted - the tests never pass without having raced."""
import time

import numpy as np
import pytest

import scenes
from devguard import Guarded
from legkilo_amd import abi, synth
from scenes import mature_oracle_map

pytestmark = pytest.mark.gpu

CAPS = dict(max_roots=1 << 16, max_nodes=1 << 17, max_point_blocks=1 << 16, max_scan_points=1 << 17)
S, N_SLOTS, N_PTS, NB = 3, 9, 2048, 4
T0 = 1.0
POSE_FIELDS = ("rot", "pos", "vel", "n_effect", "n_buckets", "n_updates")


class Content:
    """S scans with their priors, and what the oracle makes of every slot."""

    def __init__(self, name, scans, xs, Ps):
        self.name, self.scans = name, scans
        self.pts = np.ascontiguousarray(np.concatenate(scans))
        self.x = np.ascontiguousarray(np.array(xs))
        self.P = np.ascontiguousarray(np.array(Ps).reshape(len(scans), 900))
        self.want = None       # [(counts, x36)] per slot: the oracle
        self.given = None      # bits of the replay of the buffer as given
        self.sorted = None     # bits of the replay of the voxel-ordered batch


class World:
    def __init__(self, scene, oracle_lib, hip_lib):
        self.scene, self.hip_lib = scene, hip_lib
        self.o = oracle_lib.Oracle(scene.cfg(), imu_mode_only=True)
        self.blob = mature_oracle_map(self.o, scene, T0)
        self.o.set_map_insert(False)
        self.off = self.dt = None
        self.g0 = self.handle()          # LK_BATCH_ORDER_AS_GIVEN: where the reference bits come from
        self.g0.batch_order(0)
        self._cache = {}

    def handle(self):
        g = self.hip_lib.LegKiloHip(self.scene.cfg(n_slots=N_SLOTS))
        g.map_import(self.blob)
        g.init_process_cov_q()
        return g

    def scan(self, k, n_pts=N_PTS, variant=0):
        """Scan number k (its own time, seeds and prior), buckets in random order; variant: other points at the same time under the same prior."""
        tb = T0 + 1.2 + 0.37 * k
        sc = synth.dense_scan(self.scene.world, self.scene.traj, tb, self.scene.P, n=n_pts, n_buckets=NB, seed_scan=9119 + k + 1000 * variant,
                              seed_noise=8228 + k + 1000 * variant)
        off, dt = synth.buckets_of(sc)
        rng = np.random.default_rng([5150, k, n_pts, variant])
        for b in range(len(dt)):
            a, e = int(off[b]), int(off[b + 1])
            sc[a:e] = sc[a:e][rng.permutation(e - a)]
        x = synth.initial_state(self.scene.traj, tb, self.scene.P, np.random.default_rng([6160, k]), 0.02, 0.5)
        return sc, x, (off, dt)

    def content(self, name, ks, n_pts=N_PTS, variants=None, ulp=False):
        key = (name, n_pts)
        if key in self._cache:
            return self._cache[key]
        parts = [self.scan(k, n_pts, (variants or {}).get(i, 0)) for i, k in enumerate(ks)]
        for _, _, (off, dt) in parts:            # one set of bucket bounds per batch
            assert len(dt) == NB
            assert np.array_equal(off, parts[0][2][0]) and np.array_equal(dt, parts[0][2][1])
        scans = [p[0] for p in parts]
        if ulp:                                  # point 0 moved by one ulp in x: a change the sample sees
            scans[0] = scans[0].copy()
            scans[0]["x"][0] = np.nextafter(scans[0]["x"][0], np.float32(np.inf))
        c = Content(name, scans, [p[1] for p in parts], [1e-4 * np.eye(30) for _ in parts])
        c.off, c.dt = parts[0][2]
        c.n_pts = n_pts
        c.want = []
        for s, sc in enumerate(scans):
            self.o.set_state(c.x[s], c.P[s].reshape(30, 30))
            self.o.set_times(0.0, 0.0)
            po, _ = self.o.process_scan(sc, 0.0)
            c.want.append(((po.n_buckets, po.n_updates, po.n_effect), self.o.get_state()[0].copy()))
        # the preconditions, on the oracle alone: every bucket of every slot updates, so every bucket's residual launch matters
        for s, ((nbk, nup, neff), _) in enumerate(c.want):
            assert nup == NB and neff > 0, (name, s, nbk, nup, neff)
        self._bits(c)
        self._cache[key] = c
        return c

    def _bits(self, c):
        """The two sets of reference bits of a content, on the LK_BATCH_ORDER_AS_GIVEN handle: the batch as given through the asynchronous entry, and the
        synchronous replay of lk_batch_sort_by_voxel_dev's output under the same priors."""
        g, n = self.g0, len(c.scans)
        d_in, d_out = g.device_malloc(c.pts.nbytes), g.device_malloc(c.pts.nbytes)
        d_x, d_P = g.device_malloc(c.x.nbytes), g.device_malloc(c.P.nbytes)
        g.h2d(d_in, c.pts)
        g.h2d(d_x, c.x)
        g.h2d(d_P, c.P)
        out = pinned_poses(n)
        g.batch_replay_async_dev(d_in, 0, n, c.n_pts, 0.0, c.off, c.dt, d_x36=d_x, d_P900=d_P, host_out_ptr=out.ctypes.data)
        g.synchronize()
        c.given = (out.copy(), g.batch_get_states(0, n, want_P=False)[0])
        g.batch_set_priors(c.x, c.P)
        g.batch_sort_by_voxel_dev(d_in, d_out, n, c.n_pts, c.off)
        poses = g.batch_replay_dev(d_out, n, c.n_pts, 0.0, c.off, c.dt)
        c.sorted = (np.frombuffer(poses, dtype=abi.pose_dtype()).copy(), g.batch_get_states(0, n, want_P=False)[0])
        for d in (d_in, d_out, d_x, d_P):
            g.device_free(d)
        check_oracle(c, c.given[0], c.given[1])
        check_oracle(c, c.sorted[0], c.sorted[1])
        assert not same_poses(c.given[0], c.sorted[0]), c.name     # two orders of the same scans: the bits tell them apart

    def close(self):
        self.g0.close()
        self.o.close()


_PINNED = []   # (the torch tensors behind the pinned pose arrays: kept alive with the module)


def pinned_poses(n):
    """lk_pose[n] in pinned host memory: a copy into pageable memory would make the enqueue wait for the stream."""
    import torch

    t = torch.zeros(n * abi.pose_dtype().itemsize, dtype=torch.uint8).pin_memory()
    _PINNED.append(t)
    return t.numpy().view(abi.pose_dtype())


def same_poses(a, b):
    return all(np.array_equal(a[f], b[f]) for f in POSE_FIELDS)


def check_oracle(c, poses, X=None):
    """Poses (and slot states) of one replay of content c against the oracle: counts exact, state rtol 1e-8 / atol 1e-9."""
    for s, (cnt, xo) in enumerate(c.want):
        assert cnt == (int(poses[s]["n_buckets"]), int(poses[s]["n_updates"]), int(poses[s]["n_effect"])), (c.name, s)
        assert np.allclose(xo[:9], poses[s]["rot"], rtol=1e-8, atol=1e-9) and np.allclose(xo[9:12], poses[s]["pos"], rtol=1e-8, atol=1e-9), \
            (c.name, s, np.abs(xo[9:12] - poses[s]["pos"]).max())
        if X is not None:
            assert np.allclose(xo, X[s], rtol=1e-8, atol=1e-9), (c.name, s, np.abs(xo - X[s]).max())


@pytest.fixture(scope="module")
def world(oracle_lib, hip_lib):
    w = World(scenes.Scene(**CAPS), oracle_lib, hip_lib)
    yield w
    w.close()


@pytest.fixture(scope="module")
def contents(world):
    A, B, C = world.content("A", (0, 1, 2)), world.content("B", (3, 4, 5)), world.content("C", (6, 7, 8))
    for s in range(S):    # a replay of the wrong content must not pass the tolerance
        assert np.abs(A.want[s][1][9:12] - B.want[s][1][9:12]).max() > 1e-4, s
    return A, B, C


class Batch:
    """A caller's device buffer with priors in HBM, on handle g."""

    def __init__(self, g, c):
        self.g, self.c = g, c
        self.d_pts, self.d_x, self.d_P = g.device_malloc(c.pts.nbytes), g.device_malloc(c.x.nbytes), g.device_malloc(c.P.nbytes)
        self.load(c)

    def load(self, c):
        self.c = c
        self.g.h2d(self.d_pts, c.pts)
        self.g.h2d(self.d_x, c.x)
        self.g.h2d(self.d_P, c.P)

    def replay(self, ring, priors=True):
        out = pinned_poses(len(self.c.scans))
        n = len(self.c.scans)
        self.g.batch_replay_async_dev(self.d_pts, ring * n, n, self.c.n_pts, 0.0, self.c.off, self.c.dt, d_x36=self.d_x if priors else None,
                                      d_P900=self.d_P if priors else None, host_out_ptr=out.ctypes.data)
        return out

    def readback(self):
        chk = np.empty_like(self.c.pts)
        self.g.d2h(chk, self.d_pts)
        return chk

    def free(self):
        for d in (self.d_pts, self.d_x, self.d_P):
            self.g.device_free(d)


def with_copy(world, c):
    """A handle on which the library holds a voxel-ordered copy of content c's buffer: three replays, the third sorts."""
    g = world.handle()
    b = Batch(g, c)
    outs = []
    for _ in range(3):
        outs.append(b.replay(0))
        g.synchronize()
    assert g.batch_order_stats() == (1, 1, 0), g.batch_order_stats()
    assert same_poses(outs[0], c.given[0]) and same_poses(outs[1], c.given[0]) and same_poses(outs[2], c.sorted[0])
    return g, b


class Filler:
    """Bounded GPU work on the handle's main stream (torch.cuda._sleep: a spin for a number of clock ticks), timed once alone and then sized to hold the
    stream for `factor` x the host time of what has to be enqueued behind it."""

    def __init__(self, g):
        import torch

        self.torch = torch
        self.ext = torch.cuda.ExternalStream(g.stream())
        self.probe_ticks = 20_000_000
        torch.cuda._sleep(1000)                    # (loads the kernel)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.ext):
            e0.record()
            torch.cuda._sleep(self.probe_ticks)
            e1.record()
        e1.synchronize()
        self.probe_ms = e0.elapsed_time(e1)
        assert self.probe_ms > 0.5, self.probe_ms   # the spin is long enough for the event timer to resolve

    def run(self, host_s, factor=20):
        """Enqueue a filler of >= factor x host_s (at least 50 ms, at most 2 s); returns the event recorded behind it."""
        want_ms = min(max(factor * host_s * 1e3, 50.0), 2000.0)
        assert want_ms >= factor * host_s * 1e3, (host_s, "the enqueues are too slow to race a bounded filler")
        ticks = int(self.probe_ticks * want_ms / self.probe_ms) + 1
        ev = self.torch.cuda.Event()
        with self.torch.cuda.stream(self.ext):
            self.torch.cuda._sleep(ticks)
            ev.record()
        self.want_ms = want_ms
        return ev


def host_time_of_two_enqueues(b, rings):
    """Host seconds of two back-to-back enqueues of b on the given rings (the copy is current: the path the race takes), waited for afterwards;
    the slowest of three."""
    worst = None
    for _ in range(3):
        t = time.perf_counter()
        b.replay(rings[0])
        b.replay(rings[1], priors=rings[1] == 0)
        dt = time.perf_counter() - t
        b.g.synchronize()
        worst = dt if worst is None else max(worst, dt)
    return worst


def test_t1_copy_made_and_read_on_all_three_rings(world, contents):
    A = contents[0]
    g = world.handle()
    b = Batch(g, A)
    outs = [b.replay(k % 3) for k in range(6)]      # first_slot 0, S, 2S, 0, S, 2S; nothing synchronises in between
    g.synchronize()
    assert g.batch_order_stats() == (1, 1, 0), g.batch_order_stats()
    for k in (0, 1):
        assert same_poses(outs[k], A.given[0]), k
    for k in (2, 3, 4, 5):
        assert same_poses(outs[k], A.sorted[0]), k
    for k in range(6):
        check_oracle(A, outs[k])
    for ring in range(3):                            # the slots hold replays 4 to 6
        X, _ = g.batch_get_states(ring * S, S, want_P=False)
        assert np.array_equal(X, A.sorted[1]), ring
        check_oracle(A, outs[3 + ring], X)
    assert np.array_equal(b.readback().view(np.uint8), A.pts.view(np.uint8))   # the caller's buffer is never written
    b.free()
    g.close()


def test_t2_new_content_two_replays_in_flight_on_one_stream(world, contents):
    A, B = contents[0], contents[1]
    g, b = with_copy(world, A)
    fill = Filler(g)
    host_s = host_time_of_two_enqueues(b, (0, 0))
    st0 = g.batch_order_stats()
    g.synchronize()
    b.load(B)                                        # new scans in the buffer the copy was made from, B's priors
    ev = fill.run(host_s)
    t = time.perf_counter()
    o1 = b.replay(0)
    o2 = b.replay(0)
    raced_s = time.perf_counter() - t
    raced = ev.query() is False                      # the device had looked at neither replay when the second enqueue returned
    g.synchronize()
    print(f"T2: filler alone {fill.probe_ms:.2f} ms per {fill.probe_ticks} ticks; host time of two enqueues {host_s * 1e3:.3f} ms (measured), {raced_s * 1e3:.3f} ms (raced); "
          f"filler {fill.want_ms:.1f} ms = {fill.want_ms / (host_s * 1e3):.0f} x")
    assert raced, "the filler finished before the second enqueue returned: nothing raced"
    X, _ = g.batch_get_states(0, S, want_P=False)
    check_oracle(B, o1)
    check_oracle(B, o2, X)                           # the header: "that replay reads the buffer as given" - both of them
    assert same_poses(o1, B.given[0]) and same_poses(o2, B.given[0]) and np.array_equal(X, B.given[1])
    o3 = b.replay(0)
    g.synchronize()
    o4 = b.replay(0)
    g.synchronize()
    st = g.batch_order_stats()
    assert st[2] == st0[2] + 1, (st0, st)            # one sorted batch whose buffer later held other content
    assert st[1] == st0[1] + 1, (st0, st)            # ... sorted again two replays later
    check_oracle(B, o3)
    check_oracle(B, o4, g.batch_get_states(0, S, want_P=False)[0])
    assert same_poses(o3, B.given[0]) and same_poses(o4, B.sorted[0])
    assert np.array_equal(b.readback().view(np.uint8), B.pts.view(np.uint8))
    b.free()
    g.close()


def test_t3_new_content_two_replays_in_flight_on_two_rings(world, contents):
    A, B = contents[0], contents[1]
    g, b = with_copy(world, A)
    fill = Filler(g)
    x2, P2 = np.ascontiguousarray(np.concatenate([A.x, A.x])), np.ascontiguousarray(np.concatenate([A.P, A.P]))
    d_x2, d_P2 = g.device_malloc(x2.nbytes), g.device_malloc(P2.nbytes)
    g.h2d(d_x2, x2)
    g.h2d(d_P2, P2)
    g.batch_set_priors_dev(d_x2, d_P2, 2 * S)
    host_s = host_time_of_two_enqueues(b, (0, 1))    # (ring 1 without priors of its own: slots [S, 2S) keep what the replay before left - timing only)
    g.synchronize()
    b.load(B)
    g.h2d(d_x2, np.ascontiguousarray(np.concatenate([B.x, B.x])))
    g.h2d(d_P2, np.ascontiguousarray(np.concatenate([B.P, B.P])))
    g.batch_set_priors_dev(d_x2, d_P2, 2 * S)        # slots [S, 2S) armed on the main stream
    ev = fill.run(host_s)
    o1 = b.replay(0)                                 # on the main stream, behind the filler
    o2 = b.replay(1, priors=False)                   # on a side stream that waits for the main stream's event: behind the filler too
    raced = ev.query() is False
    g.synchronize()
    print(f"T3: filler alone {fill.probe_ms:.2f} ms per {fill.probe_ticks} ticks; host time of two enqueues {host_s * 1e3:.3f} ms; filler {fill.want_ms:.1f} ms = "
          f"{fill.want_ms / (host_s * 1e3):.0f} x")
    assert raced, "the filler finished before the second enqueue returned: nothing raced"
    check_oracle(B, o1, g.batch_get_states(0, S, want_P=False)[0])
    check_oracle(B, o2, g.batch_get_states(S, S, want_P=False)[0])
    assert same_poses(o1, B.given[0]) and same_poses(o2, B.given[0])
    for d in (d_x2, d_P2):
        g.device_free(d)
    b.free()
    g.close()


def test_t4_content_goes_back(world, contents):
    A, B = contents[0], contents[1]
    g, b = with_copy(world, A)
    for rnd, c in enumerate((A, B, A)):
        b.load(c)
        outs = [b.replay(0), b.replay(0)]
        g.synchronize()
        X, _ = g.batch_get_states(0, S, want_P=False)
        for k, o_ in enumerate(outs):
            check_oracle(c, o_, X if k == 1 else None)
            if rnd == 0:      # the buffer still holds what the copy was made from: the copy is read
                assert same_poses(o_, A.sorted[0]), k
            elif rnd == 1:    # other content: as given
                assert same_poses(o_, B.given[0]), k
            else:             # A again: the copy only if it is a copy of A
                assert same_poses(o_, A.given[0]) or same_poses(o_, A.sorted[0]), k
    assert g.batch_order_stats()[2] == 1, g.batch_order_stats()
    b.free()
    g.close()


def test_t5_three_buffers_two_cache_entries(world, contents):
    g = world.handle()
    bufs = [Batch(g, c) for c in contents]
    outs = [(k, bufs[k].replay(k)) for _ in range(6) for k in range(3)]
    g.synchronize()
    for k, o_ in outs:
        c = contents[k]
        check_oracle(c, o_)
        assert same_poses(o_, c.given[0]) or same_poses(o_, c.sorted[0]), c.name
    for k in range(3):
        X, _ = g.batch_get_states(k * S, S, want_P=False)
        check_oracle(contents[k], outs[-3 + k][1], X)
        assert np.array_equal(X, contents[k].given[1]) or np.array_equal(X, contents[k].sorted[1]), k
    # two buffers the handle has not seen, alternating: both are sorted, and from then on read from their copies
    two = [Batch(g, contents[1]), Batch(g, contents[2])]
    st0 = g.batch_order_stats()
    is_sorted, log = [False, False], []
    for r in range(8):
        k = r % 2
        before = g.batch_order_stats()[1]
        o_ = two[k].replay(r % 3)
        if g.batch_order_stats()[1] > before:
            is_sorted[k] = True                      # this very call made the copy: this replay and the later ones read it
        log.append((k, is_sorted[k], o_))
    g.synchronize()
    assert g.batch_order_stats()[1] == st0[1] + 2 and is_sorted == [True, True], (st0, g.batch_order_stats())
    for k, srt, o_ in log:
        c = two[k].c
        check_oracle(c, o_)
        assert same_poses(o_, c.sorted[0]) if srt else same_poses(o_, c.given[0]), (c.name, srt)
    for q in bufs + two:
        assert np.array_equal(q.readback().view(np.uint8), q.c.pts.view(np.uint8))
        q.free()
    g.close()


def test_t6_edit_outside_the_sample_and_lk_batch_changed(world, contents):
    A = contents[0]
    E = world.content("A, scan 2 replaced", (0, 1, 2), variants={2: 1})
    assert np.array_equal(E.pts[:2 * N_PTS].view(np.uint8), A.pts[:2 * N_PTS].view(np.uint8))                 # every sampled point is A's
    assert not np.allclose(E.want[2][1], A.want[2][1], rtol=1e-8, atol=1e-9)                                  # ... but slot 2's result is not
    g, b = with_copy(world, A)
    b.load(E)
    g.batch_changed()                                # what the header says to do after such an edit
    o1 = b.replay(0)
    g.synchronize()
    check_oracle(E, o1, g.batch_get_states(0, S, want_P=False)[0])
    assert same_poses(o1, E.given[0])
    b.free()
    g.close()
    # one ulp in point 0's x: sampled, so noticed without any call
    U = world.content("A, point 0 one ulp", (0, 1, 2), ulp=True)
    diff = np.flatnonzero(U.pts.view(np.uint8) != A.pts.view(np.uint8))
    assert 1 <= diff.size <= 4 and diff.max() < 4, diff
    g, b = with_copy(world, A)
    st0 = g.batch_order_stats()
    b.load(U)
    o1 = b.replay(0)
    g.synchronize()
    X, _ = g.batch_get_states(0, S, want_P=False)
    assert same_poses(o1, U.given[0]) and np.array_equal(X, U.given[1])
    check_oracle(U, o1, X)
    o2 = b.replay(0)                                 # the host learns of it at its next look
    g.synchronize()
    assert g.batch_order_stats() == (st0[0], st0[1], st0[2] + 1), (st0, g.batch_order_stats())
    assert same_poses(o2, U.given[0])
    b.free()
    g.close()


@pytest.mark.parametrize("n_pts", [2047, 2048])
def test_t7_tracking_threshold(world, n_pts):
    """S = 2: 4 094 points are below the 4 096 a batch must have to be tracked, 4 096 are not.  The caller's buffers lie between guard bands."""
    c = world.content(f"two scans of {n_pts}", (9, 10), n_pts=n_pts)
    g = world.handle()
    gp = Guarded.input(g, c.pts, offset=16, name=f"t7 d_pts {n_pts}")
    gx = Guarded.input(g, c.x, offset=8, name=f"t7 d_x36 {n_pts}")
    gP = Guarded.input(g, c.P, offset=8, name=f"t7 d_P900 {n_pts}")
    outs, stats = [], []
    for k in range(5):
        out = pinned_poses(2)
        g.batch_replay_async_dev(gp.ptr, (k % 3) * 2, 2, n_pts, 0.0, c.off, c.dt, d_x36=gx.ptr, d_P900=gP.ptr, host_out_ptr=out.ctypes.data)
        g.synchronize()
        outs.append(out)
        stats.append(g.batch_order_stats())
    for o_ in outs:
        check_oracle(c, o_)
    if n_pts == 2047:
        assert stats == [(0, 0, 0)] * 5, stats
        for o_ in outs:
            assert same_poses(o_, c.given[0])
    else:
        assert stats == [(0, 0, 0), (0, 0, 0), (1, 1, 0), (1, 1, 0), (1, 1, 0)], stats   # examined at the third replay
        assert same_poses(outs[0], c.given[0]) and same_poses(outs[1], c.given[0])
        for o_ in outs[2:]:
            assert same_poses(o_, c.sorted[0])
    for q in (gp, gx, gP):
        q.check()
        q.free()
    g.close()


def test_t8_prepare_in_as_given_mode(world, contents):
    A = contents[0]
    g = world.handle()
    b = Batch(g, A)
    g.batch_order(0)
    g.batch_set_priors(np.concatenate([A.x] * 3), np.concatenate([A.P] * 3))
    g.batch_prepare_dev(b.d_pts, S, N_PTS, A.off)    # LK_OK, and nothing is examined: no replay would read the copy
    assert g.batch_order_stats() == (0, 0, 0)
    o1 = b.replay(0)
    g.synchronize()
    assert same_poses(o1, A.given[0]) and g.batch_order_stats() == (0, 0, 0)
    g.batch_order(1)                                 # ... and nothing was kept: the usual three-replay rule
    outs = []
    for k in range(3):
        outs.append(b.replay(0))
        g.synchronize()
        assert g.batch_order_stats() == ((0, 0, 0) if k < 2 else (1, 1, 0)), (k, g.batch_order_stats())
    assert same_poses(outs[0], A.given[0]) and same_poses(outs[1], A.given[0]) and same_poses(outs[2], A.sorted[0])
    check_oracle(A, outs[2], g.batch_get_states(0, S, want_P=False)[0])
    b.free()
    g.close()
