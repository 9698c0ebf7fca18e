"""The workload the run-replay and scoring measurement tools share (replay_runs, overlay_runs, overlay_commit, runs_cloud, map_clouds, traj_ate,
traj_rpe, map_c2c, map_mme), and how they time it.  Imported, not run.

Workload: the tests' synthetic scene, a handle with a slot per run, the map (first frame + --map-scans scans replayed live), then D = --distinct
segments of K = --scans config-1 scans, each with its IMU records (only_imu_use); run r of R = --runs replays segment r % D from a perturbed prior of
its own.  The flattened tables of all runs and their device copies are made here, and the priors are drawn here, so that every tool sees the same bytes.
EventTimer, stats, both, per_launch: the HIP-event timing of a synchronous call and the library's launch profiler around one."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # scenes.py: the synthetic room / trajectory / first-frame helpers the tests use
import lk_pkg  # noqa: E402

lk_pkg.load()
import scenes  # noqa: E402
from legkilo_amd import binding, synth  # noqa: E402


def parser(json_default=""):
    """The arguments every tool of this workload takes; a tool adds its own."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=1024)
    ap.add_argument("--scans", type=int, default=4, help="scans per run")
    ap.add_argument("--distinct", type=int, default=8, help="different trajectory segments among the runs")
    ap.add_argument("--map-scans", type=int, default=3, help="scans replayed live behind the first frame before the map is frozen")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="", help="recorded in the JSON")
    ap.add_argument("--json", default=json_default)
    return ap


class Workload:
    """scan_gap: seconds between the end of a scan and the start of the next one of its run.  per_scan: draw a prior for every scan (x holds R * K
    of them, a run starts from its first scan's: x[::K]) instead of one per run (x holds R)."""

    def __init__(self, args, scan_gap=0.0, per_scan=False):
        self.R, self.K, self.D = R, K, D = args.runs, args.scans, min(args.distinct, args.runs)
        self.sc = sc = scenes.Scene()
        self.g = g = binding.LegKiloHip(sc.cfg(n_slots=R))
        self.t0 = t0 = 1.0
        x0 = scenes.init_filter(g, sc, t0)
        scenes.first_frame(g, sc, t0, x0)
        scenes.replay_vlp(g, sc, t0, args.map_scans)
        # the D segments: K scans 0.1 s + scan_gap apart, each with its IMU records
        self.seg_scans, self.seg_tb, self.seg_imu = [], [], []
        for d in range(D):
            tbs = [t0 + 0.1 * (args.map_scans + 1) + 0.37 * d + (0.1 + scan_gap) * j for j in range(K)]
            self.seg_scans.append([scenes.vlp_scan_input(sc, tb, 500 + K * d + j) for j, tb in enumerate(tbs)])
            self.seg_imu.append([synth.imu_stream(sc.traj, tb, tb + 0.1, seed=6000 + K * d + j) for j, tb in enumerate(tbs)])
            self.seg_tb.append(tbs)
        rng = np.random.default_rng(2468)
        self.seg_of = [r % D for r in range(R)]
        self.t = t = self.tables(0, K)
        self.run_off, self.scan_off, self.tb, self.n_msg, self.msg_off = t["run_off"], t["scan_off"], t["t_begin"], t["n_msg"], t["msg_off"]
        self.n_pts = len(t["pts"])
        self.d_pts, self.d_imu = self.upload(t)
        self.x = np.array([synth.initial_state(sc.traj, tb, sc.P, rng, 0.02, 0.5) for tb in (self.tb if per_scan else self.tb[::K])])
        self.P = np.tile((1e-4 * np.eye(30)).reshape(1, 900), (R, 1))

    def tables(self, lo, hi):
        """Scans lo .. hi of every run as the run entries' flat tables (binding.flatten_runs), with msg_off = where each scan's messages start."""
        pick = lambda seg: [seg[self.seg_of[r]][lo:hi] for r in range(self.R)]   # noqa: E731
        t = binding.flatten_runs(pick(self.seg_scans), pick(self.seg_tb), imus=pick(self.seg_imu))
        t["msg_off"] = np.r_[0, np.cumsum(t["n_msg"])]
        return t

    def upload(self, t):
        """Device copies of a table's points and messages: (d_pts, d_imu)."""
        d_pts, d_imu = self.g.device_malloc(t["pts"].nbytes), self.g.device_malloc(t["msgs"].nbytes)
        self.g.h2d(d_pts, t["pts"])
        self.g.h2d(d_imu, t["msgs"])
        return d_pts, d_imu

    def close(self, *more):
        """Frees the workload's device arrays and the tool's own (more), then the handle."""
        for d in (self.d_pts, self.d_imu) + more:
            self.g.device_free(d)
        self.g.close()


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def both(res):
    return dict(event_ms=stats([a for a, _ in res]), wall_ms=stats([b for _, b in res]))


class EventTimer:
    """Two HIP events on the handle's stream, from the runtime the library itself is linked against (its symbols resolve through the library's
    handle), around synchronous calls."""

    def __init__(self, g, args):
        self.hip, self.stream, self.n, self.warmup = g.L, C.c_void_p(g.stream()), args.warmup + args.reps, args.warmup
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def once(self, call):
        """(ms between two events around the call, ms of host wall time)"""
        hip, ev = self.hip, self.ev
        assert hip.hipEventRecord(ev[0], self.stream) == 0
        t1 = time.perf_counter()
        call()
        wall = time.perf_counter() - t1
        ms = C.c_float()
        assert hip.hipEventRecord(ev[1], self.stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0 and hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return float(ms.value), wall * 1e3

    def timed(self, call, before=None):
        """[(event ms, wall ms)] of the --reps timed calls behind the --warmup untimed ones; before() runs untimed in front of each."""
        res = []
        for _ in range(self.n):
            if before:
                before()
            res.append(self.once(call))
        return res[self.warmup:]

    def close(self):
        for e in self.ev:
            self.hip.hipEventDestroy(e)


def per_launch(g, call, names, reps, count=None):
    """{name: [ms of that launch in each of reps profiled calls]} from the library's launch profiler; count: how often each must have run per call."""
    per = {k: [] for k in names}
    g.profile_reset()
    g.profile_enable(True)
    try:
        for _ in range(reps):
            g.profile_reset()
            call()
            for k in names:
                n, ms = g.profile_get(k)
                assert count is None or n == count, (k, n)
                per[k].append(ms)
    finally:
        g.profile_enable(False)
    return per
