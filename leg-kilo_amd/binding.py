"""ctypes wrapper over liblegkilo_hip.so (the C-ABI of include/legkilo_hip.h).

There is no fallback: if the shared library is missing or no gfx950 device is visible the
constructor raises.  Nothing here imports oracle/.
"""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi, synth

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LEGKILO_HIP_LIB", os.path.join(_HERE, "liblegkilo_hip.so"))  # override: A/B builds

EXPORTS = sorted(abi.signatures())   # every lk_* prototype of include/legkilo_hip.h
LegKiloError = abi.LegKiloError


def build(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(_HERE, "..", "include", "legkilo_hip.h")]
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in deps):
        subprocess.check_call(["make", "-C", csrc, "-B"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LegKiloError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        # PyTorch ships its own copy of the HIP runtime.  When both copies live in one process, torch's has to come up FIRST: brought up
        # after this library has created its streams, torch.cuda fails with "No HIP GPUs are available".  So a process that has torch
        # imported (the multi-GPU replay, the device-pointer entries) gets torch's runtime initialised before the first handle exists.
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            torch.cuda.init()
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in abi.signatures().items():   # the header's types: ctypes converts and checks every argument of every call
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _messages(imus, kins, n_scans):
    """Per-scan message arrays, imus (lk_imu records) or kins (lk_kin_imu), one array per scan -> (msg_kind 0 / 1 (imus) / 2 (kins), n_msg
    uint32 [n_scans] or None, all records contiguous or None when there is none)."""
    assert imus is None or kins is None
    msgs = imus if imus is not None else kins
    if msgs is None:
        return 0, None, None
    assert len(msgs) == n_scans, "one message array per scan"
    n_msg = np.fromiter((len(m) for m in msgs), dtype=np.uint32, count=n_scans)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(m) for m in msgs if len(m)])) if n_msg.sum() else None
    return (1 if imus is not None else 2), n_msg, flat


LK_RUNS_CONTINUE = 1


def flatten_runs(runs, t_begins, imus=None, kins=None):
    """The flat tables of the run entries (lk_batch_replay_overlay_runs_dev, lk_batch_replay_runs_dev) from nested host inputs: runs = a list of
    runs, each a list of scans (lk_point arrays); t_begins, imus / kins: the same nesting (one start time, one message array per scan).  Pure:
    touches no device.  Returns a dict: run_off uint32 [R + 1], scan_off uint64 [S + 1], t_begin float64 [S], pts (all points, contiguous),
    msg_kind 0 / 1 (imus) / 2 (kins), n_msg uint32 [S] or None, msgs (all records, contiguous) or None when there is none."""
    assert imus is None or kins is None
    scans = [sc for run in runs for sc in run]
    run_off = np.r_[0, np.cumsum([len(run) for run in runs])].astype(np.uint32)
    scan_off = np.r_[0, np.cumsum([len(sc) for sc in scans])].astype(np.uint64)
    tb = np.array([t for run in t_begins for t in run], dtype=np.float64)
    assert len(tb) == len(scans), "one start time per scan"
    per_scan = lambda nested: None if nested is None else [m for run in nested for m in run]   # noqa: E731
    kind, n_msg, flat = _messages(per_scan(imus), per_scan(kins), len(scans))
    return dict(run_off=run_off, scan_off=scan_off, t_begin=tb, pts=np.ascontiguousarray(np.concatenate(scans)), msg_kind=kind, n_msg=n_msg, msgs=flat)


def pcd_file_offsets(run_off, scan_off, frames_per_file=100):
    """Which registered points go into which map file - the counting of PcdSaver::workerLoop over the run entries' tables (csrc/lk_pcd_files.h is the
    C++ twin): a file is cut after every frames_per_file scans of a run (<= 0: 100) and at each run's end for the remainder; a scan without points is
    skipped and not counted.  Returns (file_off uint64 [n_files + 1], file_run uint32 [n_files]): file f = the records file_off[f] : file_off[f + 1]
    of the run replays' d_world_out and belongs to run file_run[f].  Pure: touches no device."""
    ro = np.asarray(run_off, dtype=np.int64)
    so = np.asarray(scan_off, dtype=np.uint64)
    fpf = int(frames_per_file) if int(frames_per_file) > 0 else 100
    ends, runs = [], []
    for r in range(len(ro) - 1):
        full = np.flatnonzero(so[ro[r] + 1:ro[r + 1] + 1] != so[ro[r]:ro[r + 1]]) + ro[r]   # the run's scans that hold points
        cut = list(full[fpf - 1::fpf])                                                      # every fpf-th of them closes a file ...
        if len(full) % fpf:
            cut.append(full[-1])                                                            # ... and the run's end the remainder
        ends += [so[s + 1] for s in cut]
        runs += [r] * len(cut)
    first = so[ro[0]] if len(ro) else 0
    return np.array([first] + ends, dtype=np.uint64), np.array(runs, dtype=np.uint32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class LegKiloHip:
    def __init__(self, cfg):
        self.L = lib()
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = self.L.lk_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            msg = self.L.lk_last_error(None)
            self.h = None
            raise LegKiloError(f"lk_create failed ({rc}): {msg.decode() if msg else ''}")

    def _chk(self, rc):
        if rc != 0:
            msg = self.L.lk_last_error(self.h)
            raise LegKiloError(f"liblegkilo_hip error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            self.L.lk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @contextlib.contextmanager
    def _staged(self, *items):
        """Device memory for the length of a `with` body: per item an uploaded copy of a numpy array, or that many bytes left unwritten (an
        int), or nothing (None -> 0).  Yields the device pointers in the items' order and frees them on exit, also when the body raises."""
        dptrs = []
        try:
            for it in items:
                dptrs.append(0 if it is None else self.device_malloc(it.nbytes if isinstance(it, np.ndarray) else it))
                if isinstance(it, np.ndarray):
                    self.h2d(dptrs[-1], it)
            yield dptrs
        finally:
            for d in dptrs:
                if d:
                    self.device_free(d)

    def _export_blob(self, fn, *head):
        """The two calls of a blob export fn(*head, blob, &bytes): the size query with blob == NULL, then the blob."""
        nbytes = C.c_size_t(0)
        self._chk(fn(*head, None, C.byref(nbytes)))
        buf = np.zeros(nbytes.value, dtype=np.uint8)
        self._chk(fn(*head, _p(buf), C.byref(nbytes)))
        return buf

    # ---- ESKF surface ----
    def set_state(self, x36=None, P=None, slot=0):
        x36 = None if x36 is None else _f64(x36).reshape(36)
        P = None if P is None else _f64(P).reshape(900)
        self._chk(self.L.lk_set_state(self.h, slot, _p(x36), _p(P)))

    def get_state(self, slot=0):
        x, P = np.zeros(36), np.zeros(900)
        self._chk(self.L.lk_get_state(self.h, slot, _p(x), _p(P)))
        return x, P.reshape(30, 30)

    def set_Q(self, Q):
        Q = _f64(Q).reshape(900)
        self._chk(self.L.lk_set_Q(self.h, _p(Q)))

    def get_Q(self):
        Q = np.zeros(900)
        self._chk(self.L.lk_get_Q(self.h, _p(Q)))
        return Q.reshape(30, 30)

    def init_process_cov_q(self):
        self._chk(self.L.lk_init_process_cov_q(self.h))

    def set_times(self, last_predict_t, last_update_t, slot=0):
        self._chk(self.L.lk_set_times(self.h, slot, last_predict_t, last_update_t))

    def get_times(self, slot=0):
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.lk_get_times(self.h, slot, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_acc_norm(self, a):
        self._chk(self.L.lk_set_acc_norm(self.h, a))

    def get_acc_norm(self):
        a = C.c_double()
        self._chk(self.L.lk_get_acc_norm(self.h, C.byref(a)))
        return a.value

    def get_fx(self, dt, slot=0):
        F = np.zeros(900)
        self._chk(self.L.lk_get_fx(self.h, slot, dt, _p(F)))
        return F.reshape(30, 30)

    def get_function_f(self, dt, slot=0):
        f = np.zeros(30)
        self._chk(self.L.lk_get_function_f(self.h, slot, dt, _p(f)))
        return f

    def predict(self, dt, prop_state, prop_cov, slot=0):
        self._chk(self.L.lk_predict(self.h, slot, dt, int(prop_state), int(prop_cov)))

    def update_by_points(self, h6, z, R, slot=0):
        h6, z, R = _f64(h6), _f64(z), _f64(R)
        self._chk(self.L.lk_update_by_points(self.h, slot, _p(h6), _p(z), _p(R), len(z)))

    def update_by_imu(self, z6, R6, slot=0):
        z6, R6 = _f64(z6), _f64(R6)
        self._chk(self.L.lk_update_by_imu(self.h, slot, _p(z6), _p(R6)))

    def update_by_kin_imu(self, ki_h, ki_z, ki_R, slot=0):
        ki_h, ki_z, ki_R = _f64(ki_h), _f64(ki_z), _f64(ki_R)
        self._chk(self.L.lk_update_by_kin_imu(self.h, slot, _p(ki_h), _p(ki_z), _p(ki_R), len(ki_z)))

    # ---- VoxelMapManager surface ----
    def map_build(self, xyz_world, xyz_body):
        w = np.ascontiguousarray(xyz_world, dtype=np.float32)
        b = np.ascontiguousarray(xyz_body, dtype=np.float32)
        self._chk(self.L.lk_map_build(self.h, _p(w), _p(b), len(w)))

    def map_update(self, pw, var9):
        pw, var9 = _f64(pw), _f64(var9)
        self._chk(self.L.lk_map_update(self.h, _p(pw), _p(var9), len(pw)))

    def residuals(self, xyz_body):
        b = np.ascontiguousarray(xyz_body, dtype=np.float32)
        n = len(b)
        h6, z, R, valid = np.zeros((n, 6)), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
        self._chk(self.L.lk_residuals(self.h, _p(b), n, _p(h6), _p(z), _p(R), _p(valid)))
        return h6, z, R, valid

    def match_points(self, keys, pw, var):
        """VoxelMapManager::build_single_residual (voxel_map.cc:363-427) for n points held as pointWithVar: keys n x 3 int32, pw n x 3,
        var n x 3 x 3 -> dict(found, success, prob, normal, center, d, dis_to_plane, layer), arrays of length n."""
        keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
        n = len(keys)
        pw, var = _f64(pw).reshape(n, 3), _f64(var).reshape(n, 9)
        found, ok = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        prob, d, dis, layer = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
        normal, center = np.zeros((n, 3)), np.zeros((n, 3))
        self._chk(self.L.lk_match_points(self.h, n, _p(keys), _p(pw), _p(var), _p(found), _p(ok), _p(prob), _p(normal), _p(center),
                                         _p(d), _p(dis), _p(layer)))
        return dict(found=found.astype(bool), success=ok.astype(bool), prob=prob, normal=normal, center=center, d=d, dis_to_plane=dis, layer=layer)

    def map_stats(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.lk_map_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- local map sliding (voxel_map.cc:552-594) ----
    def map_slide(self, position, sliding_thresh=8.0, half_map_size=100):
        """VoxelMapManager::mapSliding with position_last_ = position -> (slid, n_removed)."""
        pos = _f64(position)
        slid, nrem = C.c_int32(0), C.c_uint32(0)
        self._chk(self.L.lk_map_slide(self.h, _p(pos), sliding_thresh, int(half_map_size), C.byref(slid), C.byref(nrem)))
        return bool(slid.value), int(nrem.value)

    def map_clear_outside(self, x_max, x_min, y_max, y_min, z_max, z_min):
        nrem = C.c_uint32(0)
        self._chk(self.L.lk_map_clear_outside(self.h, *(int(v) for v in (x_max, x_min, y_max, y_min, z_max, z_min)), C.byref(nrem)))
        return int(nrem.value)

    def get_last_slide_position(self):
        out = np.zeros(3)
        self._chk(self.L.lk_map_slide_position(self.h, 0, _p(out)))
        return out

    def set_last_slide_position(self, p):
        p = _f64(p).copy()
        self._chk(self.L.lk_map_slide_position(self.h, 1, _p(p)))

    def map_export(self):
        return self._export_blob(self.L.lk_map_export, self.h)

    def map_import(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._chk(self.L.lk_map_import(self.h, _p(blob), blob.size))

    def map_export_dev_size(self):
        nbytes = C.c_size_t(0)
        self._chk(self.L.lk_map_export_dev(self.h, None, C.byref(nbytes)))
        return nbytes.value

    def map_export_dev(self, d_ptr, nbytes):
        nb = C.c_size_t(nbytes)
        self._chk(self.L.lk_map_export_dev(self.h, d_ptr, C.byref(nb)))
        return nb.value

    def map_import_dev(self, d_ptr, nbytes):
        self._chk(self.L.lk_map_import_dev(self.h, d_ptr, nbytes))

    # ---- KILO path ----
    def update_points(self, t, xyz_body):
        b = np.ascontiguousarray(xyz_body, dtype=np.float32)
        n = len(b)
        w = np.zeros((n, 3), dtype=np.float32)
        inten = np.zeros(n, dtype=np.float32)
        ne = C.c_size_t(0)
        self._chk(self.L.lk_update_points(self.h, t, _p(b), n, _p(w), _p(inten), C.byref(ne)))
        return w, inten, ne.value

    def update_imu(self, imu_rec):
        a = np.ascontiguousarray(imu_rec)
        self._chk(self.L.lk_update_imu(self.h, _p(a)))

    def update_kin_imu(self, kin_rec):
        a = np.ascontiguousarray(kin_rec)
        self._chk(self.L.lk_update_kin_imu(self.h, _p(a)))

    def process_scan(self, sorted_pts, t_begin, imus=None, kins=None, want_world=False):
        pts = np.ascontiguousarray(sorted_pts)
        ni = 0 if imus is None else len(imus)
        nk = 0 if kins is None else len(kins)
        imus = None if imus is None else np.ascontiguousarray(imus)
        kins = None if kins is None else np.ascontiguousarray(kins)
        w = np.zeros((len(pts), 3), dtype=np.float32) if want_world else None
        pose = abi.lk_pose()
        self._chk(self.L.lk_process_scan(self.h, _p(pts), len(pts), t_begin, _p(imus), ni, _p(kins), nk, _p(w), C.byref(pose)))
        return pose, w

    def process_scan_dev(self, d_pts, n, t_begin, bucket_off, bucket_dt):
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        dt = _f64(bucket_dt)
        pose = abi.lk_pose()
        self._chk(self.L.lk_process_scan_dev(self.h, d_pts, n, t_begin, _p(off), _p(dt), len(dt), C.byref(pose)))
        return pose

    def run_scans_dev(self, d_pts, scan_off, t_begins, msg_kind=0, n_msg=None, d_msgs=0, slide=None, d_world=0):
        """A recorded run live on slot 0, in one call, from device-resident scans and message records (lk_run_scans_dev): scan s =
        d_pts[scan_off[s] : scan_off[s + 1]] (scan_off[0] may be non-zero), n_msg[s] records of msg_kind (1: lk_imu, 2: lk_kin_imu) per scan
        at d_msgs.  slide = (sliding_thresh, half_map_size): lk_map_slide after every scan.  d_world: device room for one 16-byte record
        per point, index-aligned with d_pts, or 0.  Returns (poses, n_slides); a LegKiloError carries n_done and the poses of the scans
        that went through."""
        so = np.ascontiguousarray(scan_off, dtype=np.uint64)
        n_scans = len(so) - 1
        tb = _f64(t_begins)
        assert len(tb) == max(n_scans, 0)
        nm = None if n_msg is None else np.ascontiguousarray(n_msg, dtype=np.uint32)
        assert nm is None or len(nm) == n_scans
        opt = None if slide is None else abi.lk_run_options(float(slide[0]), int(slide[1]), 0)
        poses = (abi.lk_pose * max(n_scans, 1))()
        n_done, n_slides = C.c_size_t(0), C.c_uint32(0)
        rc = self.L.lk_run_scans_dev(self.h, d_pts, max(n_scans, 0), _p(so), _p(tb), msg_kind, _p(nm), d_msgs,
                                     C.byref(opt) if opt is not None else None, d_world, poses, C.byref(n_done), C.byref(n_slides))
        try:
            self._chk(rc)
        except LegKiloError as e:
            e.n_done, e.poses = n_done.value, list(poses[: n_done.value])
            raise
        return list(poses[:n_scans]), n_slides.value

    def run_scans(self, scans, t_begins, imus=None, kins=None, slide=None, world=False):
        """Convenience: host scans (lk_point arrays, time-sorted, any sizes) and per-scan message arrays (imus: IMU_DTYPE, or kins:
        KIN_DTYPE) -> HBM -> run_scans_dev.  Returns (poses, worlds, n_slides): worlds = per-scan n x 3 float32 cloud_down_world
        (world=True) or None."""
        allpts = np.ascontiguousarray(np.concatenate(scans))
        scan_off = np.r_[0, np.cumsum([len(sc) for sc in scans])].astype(np.uint64)
        kind, n_msg, flat = _messages(imus, kins, len(scans))
        with self._staged(allpts, flat, 16 * len(allpts) if world else None) as (d_pts, d_msgs, d_world):
            poses, n_slides = self.run_scans_dev(d_pts, scan_off, t_begins, kind, n_msg, d_msgs, slide, d_world)
            worlds = None
            if world:
                w = np.zeros((len(allpts), 4), dtype=np.float32)
                self.d2h(w, d_world)
                worlds = [np.ascontiguousarray(w[int(a):int(b), :3]) for a, b in zip(scan_off[:-1], scan_off[1:])]
            return poses, worlds, n_slides

    # ---- sensor decode + preprocessing in front of the path ----
    def decode_scan(self, msg_bytes, n_points, layout, time_scale, filter_num, blind, header_stamp=0.0):
        """layout = dict(point_step, off_x, off_y, off_z, off_time, lidar_type)."""
        data = np.ascontiguousarray(np.frombuffer(msg_bytes, dtype=np.uint8))
        lay = abi.lk_cloud_layout(**layout)
        out = np.zeros(n_points, dtype=synth.POINT_DTYPE)
        n_out, tb, te = C.c_size_t(0), C.c_double(0), C.c_double(0)
        self._chk(self.L.lk_decode_scan(self.h, _p(data), n_points, C.byref(lay), time_scale, int(filter_num),
                                        blind, header_stamp, _p(out), C.byref(n_out), C.byref(tb), C.byref(te)))
        return out[: n_out.value], tb.value, te.value

    def decode_scan_dev(self, d_msg, n_points, layout, time_scale, filter_num, blind, header_stamp, d_out):
        """One message in HBM -> its decoded points at the device pointer d_out (room for n_points); returns (n_out, t_begin, t_end)."""
        lay = abi.lk_cloud_layout(**layout)
        n_out, tb, te = C.c_size_t(0), C.c_double(0), C.c_double(0)
        self._chk(self.L.lk_decode_scan_dev(self.h, d_msg, n_points, C.byref(lay), time_scale, int(filter_num),
                                            blind, header_stamp, d_out, C.byref(n_out), C.byref(tb), C.byref(te)))
        return n_out.value, tb.value, te.value

    def decode_scans_dev(self, d_msgs, msg_off, n_points, header_stamps, layout, time_scale, filter_num, blind, leaf, d_out):
        """A run's PointCloud2 messages in HBM (message s: n_points[s] points at byte offset msg_off[s] from d_msgs) -> decoded, voxel-grid
        filtered, time-sorted scans back to back at the device pointer d_out (room for sum(n_points) points), in one call
        (lk_decode_scans_dev).  Returns (scan_off uint64[S + 1], t_begin float64[S], t_end float64[S])."""
        mo = np.ascontiguousarray(msg_off, dtype=np.uint64)
        npts = np.ascontiguousarray(n_points, dtype=np.uint32)
        hs = _f64(header_stamps)
        S = len(mo)
        assert len(npts) == S and len(hs) == S
        lay = abi.lk_cloud_layout(**layout)
        so = np.zeros(S + 1, dtype=np.uint64)
        tb, te = np.zeros(S), np.zeros(S)
        self._chk(self.L.lk_decode_scans_dev(self.h, d_msgs, S, _p(mo), _p(npts), _p(hs), C.byref(lay), time_scale,
                                             int(filter_num), blind, leaf, d_out, _p(so), _p(tb), _p(te)))
        return so, tb, te

    def preprocess_scan(self, raw_pts, leaf):
        raw = np.ascontiguousarray(raw_pts)
        out = np.zeros(len(raw), dtype=raw.dtype)
        n_out = C.c_size_t(0)
        self._chk(self.L.lk_preprocess_scan(self.h, _p(raw), len(raw), leaf, _p(out), C.byref(n_out)))
        return out[: n_out.value]

    def preprocess_scan_dev(self, d_raw, n_raw, leaf, d_out):
        n_out = C.c_size_t(0)
        self._chk(self.L.lk_preprocess_scan_dev(self.h, d_raw, n_raw, leaf, d_out, C.byref(n_out)))
        return n_out.value

    def process_raw_scan(self, raw_pts, leaf, t_begin, imus=None, kins=None):
        raw = np.ascontiguousarray(raw_pts)
        ni = 0 if imus is None else len(imus)
        nk = 0 if kins is None else len(kins)
        imus = None if imus is None else np.ascontiguousarray(imus)
        kins = None if kins is None else np.ascontiguousarray(kins)
        pose = abi.lk_pose()
        nd = C.c_size_t(0)
        self._chk(self.L.lk_process_raw_scan(self.h, _p(raw), len(raw), leaf, t_begin, _p(imus), ni, _p(kins), nk, C.byref(nd), C.byref(pose)))
        return pose, nd.value

    # ---- batch replay ----
    def batch_set_priors(self, x36, P900):
        x36 = _f64(x36).reshape(-1, 36)
        P900 = _f64(P900).reshape(-1, 900)
        assert len(x36) == len(P900)
        self._chk(self.L.lk_batch_set_priors(self.h, _p(x36), _p(P900), len(x36)))

    def batch_set_priors_dev(self, d_x36, d_P900, n_scans):
        """Priors already in HBM (device pointers to n_scans x 36 and n_scans x 900 doubles); asynchronous."""
        self._chk(self.L.lk_batch_set_priors_dev(self.h, d_x36, d_P900, n_scans))

    def batch_get_states(self, first_slot, n, want_P=True):
        """State [n, 36] and covariance [n, 30, 30] of the filter slots first_slot .. first_slot + n (one gather kernel)."""
        x = np.zeros((n, 36))
        P = np.zeros((n, 900)) if want_P else None
        self._chk(self.L.lk_batch_get_states(self.h, first_slot, n, _p(x), _p(P)))
        return x, (P.reshape(n, 30, 30) if want_P else None)

    def batch_get_states_dev(self, first_slot, n, d_x36, d_P900):
        """The same into device buffers (pointers or 0), asynchronous on the handle's stream."""
        self._chk(self.L.lk_batch_get_states_dev(self.h, first_slot, n, d_x36, d_P900))

    def batch_replay_dev(self, d_pts, n_scans, n_pts, t_begin, bucket_off, bucket_dt, want_poses=True):
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        dt = _f64(bucket_dt)
        poses = (abi.lk_pose * n_scans)() if want_poses else None
        self._chk(self.L.lk_batch_replay_dev(self.h, d_pts, n_scans, n_pts, t_begin, _p(off), _p(dt), len(dt), poses))
        return poses

    def batch_residuals_dev(self, d_pts, n_scans, n_pts, d_rows8, d_valid):
        """Config 2 for a device-resident batch (lk_batch_residuals_dev): residual rows of n_scans x n_pts points, scan s under the current state of
        slot s, written to the device buffers d_rows8 [n][8] float64 = (h0..h5, z, R) per point and d_valid (uint8).  Asynchronous on the handle's stream."""
        self._chk(self.L.lk_batch_residuals_dev(self.h, d_pts, n_scans, n_pts, d_rows8, d_valid))

    def batch_order(self, mode):
        """0: replay every device-resident batch as given; 1 (default): the frozen-map batch entries keep a voxel-ordered copy of a batch they see (lk_batch_order)."""
        self._chk(self.L.lk_batch_order(self.h, int(mode)))

    def batch_prepare_dev(self, d_pts, n_scans, n_pts, bucket_off):
        """Make the voxel-ordered copy of a batch NOW (priors armed first) instead of at its third replay (lk_batch_prepare_dev); does nothing
        under batch_order(0), where no replay would read it."""
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        self._chk(self.L.lk_batch_prepare_dev(self.h, d_pts, n_scans, n_pts, _p(off), len(off) - 1))

    def batch_changed(self):
        self._chk(self.L.lk_batch_changed(self.h))

    def batch_order_stats(self):
        """(batches examined at first sight, of those sorted into a copy, replays that found new content in a known buffer)."""
        out = np.zeros(3, dtype=np.uint64)
        self._chk(self.L.lk_batch_order_stats(self.h, _p(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def batch_sort_by_voxel_dev(self, d_in, d_out, n_scans, n_pts, bucket_off):
        """Every bucket of every scan of a device-resident batch into root-voxel order under the slots' prior poses (lk_batch_sort_by_voxel_dev):
        d_out = the same scans, a residual wave's points a handful of voxels apart.  Priors first (batch_set_priors(_dev))."""
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        self._chk(self.L.lk_batch_sort_by_voxel_dev(self.h, d_in, d_out, n_scans, n_pts, _p(off), len(off) - 1))

    def batch_replay_async_dev(self, d_pts, first_slot, n_scans, n_pts, t_begin, bucket_off, bucket_dt, d_x36=None, d_P900=None,
                               host_out_ptr=None):
        """Enqueue a batch on slots [first_slot, first_slot + n_scans) without synchronising (alternate the slot range
        between consecutive batches to double-buffer); poses land in the PINNED host buffer at host_out_ptr once the
        batch's stream gets there (synchronize() waits for everything)."""
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        dt = _f64(bucket_dt)
        self._chk(self.L.lk_batch_replay_async_dev(self.h, d_pts, first_slot, n_scans, n_pts, t_begin, _p(off), _p(dt), len(dt), d_x36, d_P900,
                                                   host_out_ptr))

    def batch_replay_overlay_dev(self, d_pts, n_scans, n_pts, t_begin, bucket_off, bucket_dt, want_poses=True):
        """Batch replay WITH the map insert: every scan on its own copy-on-write overlay of the handle's map (lk_batch_replay_overlay_dev)."""
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        dt = _f64(bucket_dt)
        poses = (abi.lk_pose * n_scans)() if want_poses else None
        self._chk(self.L.lk_batch_replay_overlay_dev(self.h, d_pts, n_scans, n_pts, t_begin, _p(off), _p(dt), len(dt), poses))
        return poses

    def batch_replay_overlay(self, scans, t_begin, bucket_off, bucket_dt):
        """Convenience: equally shaped host scans (lk_point arrays, time-sorted, one bucket table) -> HBM -> overlay replay on slots
        [0, len(scans)); priors are whatever batch_set_priors put into those slots.  Returns the poses."""
        allpts = np.ascontiguousarray(np.concatenate(scans))
        n_pts = len(scans[0])
        assert all(len(sc) == n_pts for sc in scans), "the overlay batch entry takes equally shaped scans (ragged: lk_batch_replay_overlay_ragged_dev)"
        with self._staged(allpts) as (d,):
            return self.batch_replay_overlay_dev(d, len(scans), n_pts, t_begin, bucket_off, bucket_dt)

    def batch_replay_overlay_ragged_dev(self, d_pts, tables, want_poses=True):
        """Ragged batch WITH the map insert on slots [0, n_scans): `tables` from ragged_tables() (with imus= or kins= for the messages between
        the buckets); every scan on its own copy-on-write overlay of the handle's map (lk_batch_replay_overlay_ragged_dev)."""
        t = tables
        n_scans = t["n_scans"]
        poses = (abi.lk_pose * n_scans)() if want_poses else None
        kind, n_msg, msgs = self._ragged_messages(t)
        self._chk(self.L.lk_batch_replay_overlay_ragged_dev(self.h, d_pts, n_scans, _p(t["scan_off"]), _p(t["n_buckets"]), _p(t["bucket_off"]),
                                                            _p(t["bucket_dt"]), _p(t["t_begin"]), _p(n_msg), _p(msgs), kind, poses))
        return poses

    def batch_replay_overlay_ragged(self, scans, t_begins, xs=None, Ps=None, imus=None, kins=None):
        """Convenience: host scans (lk_point arrays, time-sorted, any sizes) -> HBM, buckets = runs of equal curvature (KILO.cc:375-378),
        optional priors and per-scan messages, ragged replay WITH insert.  Returns the poses."""
        if xs is not None:
            self.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        allpts = np.ascontiguousarray(np.concatenate(scans))
        scan_off = np.r_[0, np.cumsum([len(sc) for sc in scans])]
        tabs = [synth.buckets_of(sc) for sc in scans]
        tables = self.ragged_tables(scan_off, [t[0] for t in tabs], [t[1] for t in tabs], t_begins, imus, kins)
        with self._staged(allpts) as (d,):
            return self.batch_replay_overlay_ragged_dev(d, tables)

    def batch_replay_overlay_runs_dev(self, d_pts, run_off, scan_off, t_begins, msg_kind=0, n_msg=None, d_msgs=0, want_poses=True):
        """Whole recorded runs WITH the map insert, run r on slot r (lk_batch_replay_overlay_runs_dev): run r = the scans run_off[r] : run_off[r + 1],
        scan s = d_pts[scan_off[s] : scan_off[s + 1]] with n_msg[s] records of msg_kind (1: lk_imu, 2: lk_kin_imu) at d_msgs - all in HBM, the
        bucket tables are built there.  State, covariance, times and overlay of a slot survive its run's scan boundaries.  Returns one pose per
        SCAN (counters of that scan alone); batch_get_states / overlay_export(r) give a run's final state and overlay."""
        return self._runs_call(self.L.lk_batch_replay_overlay_runs_dev, d_pts, run_off, scan_off, t_begins, msg_kind, n_msg, d_msgs, want_poses)

    def _runs_call(self, fn, d_pts, run_off, scan_off, t_begins, msg_kind, n_msg, d_msgs, want_poses, flags=(), tail=()):
        """What the four run exports share - the run tables (run_off uint32, scan_off uint64, t_begin float64, n_msg uint32 or None) and the pose
        array: fn(handle, points, tables, messages, *flags, poses, *tail).  Returns the poses, one per scan, or None."""
        ro = np.ascontiguousarray(run_off, dtype=np.uint32)
        so = np.ascontiguousarray(scan_off, dtype=np.uint64)
        n_scans = len(so) - 1
        tb = _f64(t_begins)
        assert len(tb) == n_scans and len(ro) >= 1
        nm = None if n_msg is None else np.ascontiguousarray(n_msg, dtype=np.uint32)
        assert nm is None or len(nm) == n_scans
        poses = (abi.lk_pose * max(n_scans, 1))() if want_poses else None
        self._chk(fn(self.h, d_pts, len(ro) - 1, _p(ro), _p(so), _p(tb), msg_kind, _p(nm), d_msgs, *flags, poses, *tail))
        return list(poses[:n_scans]) if want_poses else None

    def _runs_cloud_call(self, overlay, d_pts, run_off, scan_off, t_begins, msg_kind, n_msg, d_msgs, flags, want_poses, d_world, want_offsets):
        """The two _cloud entries' call: (poses or None, scan_bucket_off uint32 [n_scans + 1] or None)."""
        sbo = np.zeros(len(scan_off), dtype=np.uint32) if want_offsets else None
        fn, fl = (self.L.lk_batch_replay_overlay_runs_cloud_dev, ()) if overlay else (self.L.lk_batch_replay_runs_cloud_dev, (flags,))
        return self._runs_call(fn, d_pts, run_off, scan_off, t_begins, msg_kind, n_msg, d_msgs, want_poses, fl, (d_world, _p(sbo))), sbo

    def batch_replay_runs_cloud_dev(self, d_pts, run_off, scan_off, t_begins, msg_kind=0, n_msg=None, d_msgs=0, cont=False, want_poses=True, flags=None,
                                    d_world=0, want_offsets=True):
        """batch_replay_runs_dev with what KILO::process returns beside the pose (lk_batch_replay_runs_cloud_dev): d_world - device pointer (16-byte
        aligned, 0: none) to one x y z intensity float record per point of d_pts, each point under the state after ITS time bucket, intensity 255 where
        that bucket updated; want_offsets: the scans' record ranges in the handle's bucket table (runs_bucket_poses).  Either output makes the call
        record the table; with neither this is batch_replay_runs_dev.  Returns (poses, scan_bucket_off or None)."""
        fl = (LK_RUNS_CONTINUE if cont else 0) if flags is None else int(flags)
        return self._runs_cloud_call(False, d_pts, run_off, scan_off, t_begins, msg_kind, n_msg, d_msgs, fl, want_poses, d_world, want_offsets)

    def batch_replay_overlay_runs_cloud_dev(self, d_pts, run_off, scan_off, t_begins, msg_kind=0, n_msg=None, d_msgs=0, want_poses=True, d_world=0,
                                            want_offsets=True):
        """batch_replay_overlay_runs_dev with the registered cloud and the bucket table (lk_batch_replay_overlay_runs_cloud_dev): outputs as for
        batch_replay_runs_cloud_dev.  Returns (poses, scan_bucket_off or None)."""
        return self._runs_cloud_call(True, d_pts, run_off, scan_off, t_begins, msg_kind, n_msg, d_msgs, 0, want_poses, d_world, want_offsets)

    def runs_bucket_poses_dev(self, first_bucket, n, d_out):
        """Records first_bucket : first_bucket + n of the last _cloud run replay's bucket table -> device memory at d_out (lk_runs_bucket_poses_dev)."""
        self._chk(self.L.lk_runs_bucket_poses_dev(self.h, first_bucket, n, d_out))

    def runs_bucket_poses(self, first_bucket, n):
        """The same records as a numpy array of abi.bucket_pose_dtype() (lk_runs_bucket_poses)."""
        out = np.zeros(n, dtype=abi.bucket_pose_dtype())
        self._chk(self.L.lk_runs_bucket_poses(self.h, first_bucket, n, _p(out)))
        return out

    def _traj_call(self, fn, dtype, est, est_off, gt, gt_off, tail, bit, on, flags, out=None):
        """What the four trajectory exports share - both offset tables, the flag rule (`bit` when `on`, unless `flags` states the word itself) and
        the records: fn(handle, n, *est, est_off, *gt, gt_off, *tail, flags, records).  Returns the n records."""
        eo = np.ascontiguousarray(est_off, dtype=np.uint64)
        go = np.ascontiguousarray(gt_off, dtype=np.uint64)
        n = max(len(eo) - 1, 0)
        assert len(go) == len(eo)
        res = np.zeros(max(n, 1), dtype=dtype) if out is None else out
        fl = (bit if on else 0) if flags is None else int(flags)
        self._chk(fn(self.h, n, *est, _p(eo), *gt, _p(go), *tail, fl, _p(res)))
        return res[:n]

    def traj_ate_dev(self, d_est_t, d_est_pos, est_stride, est_off, d_gt_t, d_gt_pos, gt_stride, gt_off, max_dt, align=False, flags=None, out=None):
        """Absolute trajectory error of len(est_off) - 1 trajectories against ground truth, all in device memory (lk_traj_ate_dev): d_*_t / d_*_pos -
        device pointers to the first sample's stamp and position, sample k `stride` bytes further on; est_off / gt_off - the trajectories' sample
        ranges.  Pairs by nearest stamp within max_dt, align: the best rigid motion removed first.  Returns abi.ate_dtype() records, one per
        trajectory (out: an array of that dtype to write into instead - n_traj records of it are written)."""
        return self._traj_call(self.L.lk_traj_ate_dev, abi.ate_dtype(), (d_est_t, d_est_pos, est_stride), est_off, (d_gt_t, d_gt_pos, gt_stride), gt_off,
                               (max_dt,), abi.LK_ATE_ALIGN, align, flags, out)

    def runs_ate_dev(self, run_bucket_off, d_gt_t, d_gt_pos, gt_stride, gt_off, max_dt, align=False, flags=None):
        """The same with the estimate read from the bucket table of the last _cloud run replay (lk_runs_ate_dev): run r = the records
        run_bucket_off[r] : run_bucket_off[r + 1] (scan_bucket_off[run_off]); the ground truth in device memory."""
        return self._traj_call(self.L.lk_runs_ate_dev, abi.ate_dtype(), (), run_bucket_off, (d_gt_t, d_gt_pos, gt_stride), gt_off, (max_dt,),
                               abi.LK_ATE_ALIGN, align, flags)

    def runs_ate(self, run_bucket_off, gt_t, gt_pos, gt_off, max_dt, align=False):
        """runs_ate_dev with the ground truth taken from the host: gt_t [m], gt_pos [m, 3] are uploaded as one packed [t x y z] table (stride 32) for
        the call.  What the windowed-mapping recipe chooses a slot with: replay, runs_ate, overlay_commit(argmin rmse)."""
        gt = np.ascontiguousarray(np.concatenate([_f64(gt_t).reshape(-1, 1), _f64(gt_pos).reshape(-1, 3)], axis=1))
        with self._staged(gt if gt.nbytes else 32) as (d_gt,):   # an empty table still gets a pointer the entry accepts
            return self.runs_ate_dev(run_bucket_off, d_gt, d_gt + 8, 32, gt_off, max_dt, align)

    def traj_rpe_dev(self, d_est_t, d_est_pos, d_est_rot, est_stride, est_off, d_gt_t, d_gt_pos, d_gt_rot, gt_stride, gt_off, max_dt, delta, by_index=False,
                     flags=None, out=None):
        """Relative pose error of len(est_off) - 1 trajectories against ground truth, all in device memory (lk_traj_rpe_dev): traj_ate_dev's tables
        with a third pointer per side, d_*_rot - the first sample's nine row-major doubles, body to world.  A step reaches from sample i to the
        first later sample at least `delta` seconds on (by_index: `delta` samples on); it is scored when both ends pair within max_dt.  Returns
        abi.rpe_dtype() records, one per trajectory (out: an array of that dtype to write into instead)."""
        return self._traj_call(self.L.lk_traj_rpe_dev, abi.rpe_dtype(), (d_est_t, d_est_pos, d_est_rot, est_stride), est_off,
                               (d_gt_t, d_gt_pos, d_gt_rot, gt_stride), gt_off, (max_dt, delta), abi.LK_RPE_INDEX, by_index, flags, out)

    def runs_rpe_dev(self, run_bucket_off, d_gt_t, d_gt_pos, d_gt_rot, gt_stride, gt_off, max_dt, delta, by_index=False, flags=None):
        """The same with the estimate read from the bucket table of the last _cloud run replay (lk_runs_rpe_dev): run r = the records
        run_bucket_off[r] : run_bucket_off[r + 1] (scan_bucket_off[run_off]); the ground truth in device memory."""
        return self._traj_call(self.L.lk_runs_rpe_dev, abi.rpe_dtype(), (), run_bucket_off, (d_gt_t, d_gt_pos, d_gt_rot, gt_stride), gt_off, (max_dt, delta),
                               abi.LK_RPE_INDEX, by_index, flags)

    def _c2c_call(self, fn, query, q_off, ref, r_off, pairs, max_dist, thr, nn_idx, nn_d2, want_nn_off, mid=(), want_c2c=True):
        """What the C2C and alignment exports share - the host tables and the records: fn(handle, query, tables, ref, tables, pairs, max_dist, thr,
        *mid, records, nn arrays); mid: what the alignment entries take in front of the lk_c2c records, which they accept as NULL (want_c2c False).
        Returns (records, nn_off or None)."""
        qo = np.ascontiguousarray(q_off, dtype=np.uint64)
        ro = np.ascontiguousarray(r_off, dtype=np.uint64)
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        pq, pref = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        th = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)
        res = np.zeros(max(len(pr), 1), dtype=abi.c2c_dtype())
        nn_off = np.zeros(len(pr) + 1, dtype=np.uint64) if want_nn_off else None
        self._chk(fn(self.h, query, max(len(qo) - 1, 0), _p(qo), ref, max(len(ro) - 1, 0), _p(ro), len(pr), _p(pq), _p(pref), max_dist,
                     _p(th) if len(th) else None, len(th), *mid, _p(res) if want_c2c else None, nn_idx, nn_d2, _p(nn_off)))
        return res[:len(pr)], nn_off

    def clouds_c2c_dev(self, d_query, q_off, d_ref, r_off, pairs, max_dist, thr=(), d_nn_idx=0, d_nn_d2=0):
        """Cloud-to-cloud nearest-neighbour distance of many pairs of clouds in device memory (lk_clouds_c2c_dev): cloud c of a side = the 16-byte
        x y z w records off[c] : off[c + 1] at its device pointer (a run replay's d_world, downsample_clouds_dev's d_out with its out_off - both
        sides may be the same buffer); pairs [n, 2] = (query cloud, reference cloud).  A query point is matched when its nearest reference point
        lies within max_dist; thr: up to four thresholds <= max_dist counted in n_within.  d_nn_idx / d_nn_d2: device pointers (0: none) that take
        the neighbour's index in its cloud and the squared distance per pair and query point.  Returns (abi.c2c_dtype() records, one per pair,
        nn_off uint64 [n + 1]: pair k's entries are nn_off[k] : nn_off[k + 1]); cloudmetrics.c2c is the numpy statement, cloudmetrics.fscore
        combines the two directions."""
        return self._c2c_call(self.L.lk_clouds_c2c_dev, d_query, q_off, d_ref, r_off, pairs, max_dist, thr, d_nn_idx or None, d_nn_d2 or None, True)

    def clouds_c2c(self, query, q_off, ref, r_off, pairs, max_dist, thr=(), want_nn=False):
        """The same with both sides in host memory (lk_clouds_c2c): query, ref float32 [n, 4] (x y z w records).  Returns (records, nn_off), with
        want_nn (records, nn_off, nn_idx uint32, nn_d2 float64)."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 4)
        r = np.ascontiguousarray(ref, dtype=np.float32).reshape(-1, 4)
        if not want_nn:
            return self._c2c_call(self.L.lk_clouds_c2c, _p(q), q_off, _p(r), r_off, pairs, max_dist, thr, None, None, True)
        qo = np.asarray(q_off, dtype=np.uint64)
        total = int(sum(int(qo[a + 1] - qo[a]) for a in np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[:, 0]))
        idx, d2 = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.float64)
        res, nn_off = self._c2c_call(self.L.lk_clouds_c2c, _p(q), q_off, _p(r), r_off, pairs, max_dist, thr, _p(idx), _p(d2), True)
        return res, nn_off, idx[:total], d2[:total]

    def _align_call(self, fn, query, q_off, ref, r_off, pairs, max_dist, thr, T0, max_iter, eps_rot, eps_trans, nn_idx, nn_d2, want_c2c):
        """What the two alignment exports share on top of _c2c_call: T0 as n rows of 12 doubles (R row-major, then t; None: the identity) and
        the lk_align records.  Returns (align records, lk_c2c records or None, nn_off)."""
        n = len(np.asarray(pairs).reshape(-1, 2))
        t0 = None if T0 is None else np.ascontiguousarray(T0, dtype=np.float64).reshape(-1, 12)
        assert t0 is None or len(t0) == n, "T0: one row of 12 doubles per pair"
        out = np.zeros(max(n, 1), dtype=abi.align_dtype())
        mid = (_p(t0) if t0 is not None else None, int(max_iter), float(eps_rot), float(eps_trans), _p(out))
        res, nn_off = self._c2c_call(fn, query, q_off, ref, r_off, pairs, max_dist, thr, nn_idx, nn_d2, True, mid, want_c2c)
        return out[:n], (res if want_c2c else None), nn_off

    def clouds_align_dev(self, d_query, q_off, d_ref, r_off, pairs, max_dist, T0=None, max_iter=30, eps_rot=1e-6, eps_trans=1e-6, thr=(), d_nn_idx=0,
                         d_nn_d2=0, want_c2c=True):
        """Rigid alignment (point-to-point ICP) of many pairs of clouds in device memory (lk_clouds_align_dev): clouds_c2c_dev's clouds, tables and
        pairs; per pair T = (R, t) with r ~ R q + t starts as T0[k] (12 doubles, R row-major then t; None: the identity) and takes up to max_iter
        solves, each from the matches of a search under the current T, until a solve moves by no more than eps_rot (radians) and eps_trans
        (metres).  Returns (abi.align_dtype() records, lk_c2c records of the final search or None, nn_off); d_nn_idx / d_nn_d2 take the final
        search's neighbours.  cloudmetrics.align is the numpy statement; clouds_transform_dev writes the moved clouds."""
        return self._align_call(self.L.lk_clouds_align_dev, d_query, q_off, d_ref, r_off, pairs, max_dist, thr, T0, max_iter, eps_rot, eps_trans,
                                d_nn_idx or None, d_nn_d2 or None, want_c2c)

    def clouds_align(self, query, q_off, ref, r_off, pairs, max_dist, T0=None, max_iter=30, eps_rot=1e-6, eps_trans=1e-6, thr=(), want_nn=False):
        """The same with both sides in host memory (lk_clouds_align): query, ref float32 [n, 4].  Returns (align records, lk_c2c records, nn_off),
        with want_nn (..., nn_idx uint32, nn_d2 float64)."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 4)
        r = np.ascontiguousarray(ref, dtype=np.float32).reshape(-1, 4)
        if not want_nn:
            return self._align_call(self.L.lk_clouds_align, _p(q), q_off, _p(r), r_off, pairs, max_dist, thr, T0, max_iter, eps_rot, eps_trans, None, None, True)
        qo = np.asarray(q_off, dtype=np.uint64)
        total = int(sum(int(qo[a + 1] - qo[a]) for a in np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[:, 0]))
        idx, d2 = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.float64)
        out, res, nn_off = self._align_call(self.L.lk_clouds_align, _p(q), q_off, _p(r), r_off, pairs, max_dist, thr, T0, max_iter, eps_rot, eps_trans,
                                            _p(idx), _p(d2), True)
        return out, res, nn_off, idx[:total], d2[:total]

    def _align_plane_call(self, fn, query, q_off, ref, r_off, normals, pairs, max_dist, thr, T0, max_iter, eps_rot, eps_trans, nn_idx, nn_d2, want_c2c):
        """What the two point-to-plane exports share on top of _c2c_call: _align_call's T0 and lk_align records, the reference normals and the
        lk_align_plane records.  Returns (align records, plane records, lk_c2c records or None, nn_off)."""
        n = len(np.asarray(pairs).reshape(-1, 2))
        t0 = None if T0 is None else np.ascontiguousarray(T0, dtype=np.float64).reshape(-1, 12)
        assert t0 is None or len(t0) == n, "T0: one row of 12 doubles per pair"
        out = np.zeros(max(n, 1), dtype=abi.align_dtype())
        pl = np.zeros(max(n, 1), dtype=abi.align_plane_dtype())
        mid = (_p(t0) if t0 is not None else None, int(max_iter), float(eps_rot), float(eps_trans), normals, _p(out), _p(pl))
        res, nn_off = self._c2c_call(fn, query, q_off, ref, r_off, pairs, max_dist, thr, nn_idx, nn_d2, True, mid, want_c2c)
        return out[:n], pl[:n], (res if want_c2c else None), nn_off

    def clouds_align_plane_dev(self, d_query, q_off, d_ref, r_off, d_ref_normals, pairs, max_dist, T0=None, max_iter=30, eps_rot=1e-6, eps_trans=1e-6, thr=(),
                               d_nn_idx=0, d_nn_d2=0, want_c2c=True):
        """Point-to-plane alignment of many pairs of clouds in device memory (lk_clouds_align_plane_dev): clouds_align_dev's arguments and
        d_ref_normals, one 16-byte nx ny nz w record per reference record at the same index as d_ref (clouds_normals_dev writes them; a record
        with a non-finite component has no plane).  Returns (abi.align_dtype() records, abi.align_plane_dtype() records, lk_c2c records of the
        final search or None, nn_off).  cloudmetrics.align_plane is the numpy statement."""
        return self._align_plane_call(self.L.lk_clouds_align_plane_dev, d_query, q_off, d_ref, r_off, d_ref_normals or None, pairs, max_dist, thr, T0, max_iter,
                                      eps_rot, eps_trans, d_nn_idx or None, d_nn_d2 or None, want_c2c)

    def clouds_align_plane(self, query, q_off, ref, r_off, ref_normals, pairs, max_dist, T0=None, max_iter=30, eps_rot=1e-6, eps_trans=1e-6, thr=(), want_nn=False):
        """The same with both sides and the normals in host memory (lk_clouds_align_plane): float32 [n, 4] each.  Returns (align records, plane
        records, lk_c2c records, nn_off), with want_nn (..., nn_idx uint32, nn_d2 float64)."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 4)
        r = np.ascontiguousarray(ref, dtype=np.float32).reshape(-1, 4)
        nr = np.ascontiguousarray(ref_normals, dtype=np.float32).reshape(-1, 4)
        assert len(nr) == len(r), "ref_normals: one record per reference record"
        if not want_nn:
            return self._align_plane_call(self.L.lk_clouds_align_plane, _p(q), q_off, _p(r), r_off, _p(nr), pairs, max_dist, thr, T0, max_iter, eps_rot, eps_trans,
                                          None, None, True)
        qo = np.asarray(q_off, dtype=np.uint64)
        total = int(sum(int(qo[a + 1] - qo[a]) for a in np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[:, 0]))
        idx, d2 = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.float64)
        out, pl, res, nn_off = self._align_plane_call(self.L.lk_clouds_align_plane, _p(q), q_off, _p(r), r_off, _p(nr), pairs, max_dist, thr, T0, max_iter, eps_rot,
                                                      eps_trans, _p(idx), _p(d2), True)
        return out, pl, res, nn_off, idx[:total], d2[:total]

    def _normals_call(self, fn, clouds, off, radius, min_pts, min_planarity, normals):
        o = np.ascontiguousarray(off, dtype=np.uint64)
        n = max(len(o) - 1, 0)
        res = np.zeros(max(n, 1), dtype=abi.normals_dtype())
        self._chk(fn(self.h, clouds, n, _p(o), radius, min_pts, min_planarity, _p(res), normals))
        return res[:n]

    def clouds_normals_dev(self, d_clouds, off, radius, d_normals, min_pts=5, min_planarity=0.0):
        """Per-point normals of many clouds in device memory (lk_clouds_normals_dev): clouds_mme_dev's clouds, table, radius and neighbourhoods; record
        off[c] + i gets (nx, ny, nz, planarity) float32 at entry off[c] - off[0] + i of d_normals - NaN in nx ny nz where the point has fewer than
        min_pts (>= 3) neighbours or a planarity below min_planarity.  Returns abi.normals_dtype() records, one per cloud; cloudmetrics.normals is
        the numpy statement."""
        return self._normals_call(self.L.lk_clouds_normals_dev, d_clouds, off, radius, min_pts, min_planarity, d_normals or None)

    def clouds_normals(self, clouds, off, radius, min_pts=5, min_planarity=0.0):
        """The same with the clouds in host memory (lk_clouds_normals): clouds float32 [n, 4].  Returns (records, normals float32 [total, 4])."""
        c = np.ascontiguousarray(clouds, dtype=np.float32).reshape(-1, 4)
        o = np.asarray(off, dtype=np.uint64)
        total = int(o[-1] - o[0]) if len(o) else 0
        nr = np.zeros((max(total, 1), 4), dtype=np.float32)
        res = self._normals_call(self.L.lk_clouds_normals, _p(c), off, radius, min_pts, min_planarity, _p(nr))
        return res, nr[:total]

    def clouds_transform_dev(self, d_in, off, T, d_out):
        """Moved clouds in device memory (lk_clouds_transform_dev): record off[c] + i of d_in goes to entry off[c] - off[0] + i of d_out with x y z
        moved under T[c] (12 doubles, R row-major then t) in float64 and rounded once to float32, w copied.  d_out may be d_in + 16 * off[0] bytes
        (in place).  cloudmetrics.transform is the numpy statement."""
        o = np.ascontiguousarray(off, dtype=np.uint64)
        t = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 12)
        assert len(t) == max(len(o) - 1, 0), "T: one row of 12 doubles per cloud"
        self._chk(self.L.lk_clouds_transform_dev(self.h, d_in, max(len(o) - 1, 0), _p(o), _p(t) if len(t) else None, d_out))

    def _mme_call(self, fn, clouds, off, radius, min_pts, n_arr, h_arr, lmin_arr):
        """What the two MME exports share - the offset table and the records: fn(handle, clouds, table, radius, min_pts, records, per-point arrays).
        Returns the records."""
        o = np.ascontiguousarray(off, dtype=np.uint64)
        n = max(len(o) - 1, 0)
        res = np.zeros(max(n, 1), dtype=abi.mme_dtype())
        self._chk(fn(self.h, clouds, n, _p(o), radius, min_pts, _p(res), n_arr, h_arr, lmin_arr))
        return res[:n]

    def clouds_mme_dev(self, d_clouds, off, radius, min_pts=5, d_n=0, d_h=0, d_lmin=0):
        """Mean map entropy and mean plane variance of many clouds in device memory, no reference needed (lk_clouds_mme_dev): cloud c = the 16-byte
        x y z w records off[c] : off[c + 1] at the device pointer d_clouds (a run replay's d_world, downsample_clouds_dev's d_out with its out_off).
        A point's neighbourhood is every record of its cloud within `radius`, itself included; with at least min_pts (>= 4) of them it is dense and
        gets lmin, and h unless its covariance is flat.  d_n / d_h / d_lmin: device pointers (0: none, each on its own) that take n_i uint32, h_i and
        lmin_i float64 per record, entry off[c] - off[0] + i.  Returns abi.mme_dtype() records, one per cloud; cloudmetrics.mme is the numpy
        statement."""
        return self._mme_call(self.L.lk_clouds_mme_dev, d_clouds, off, radius, min_pts, d_n or None, d_h or None, d_lmin or None)

    def clouds_mme(self, clouds, off, radius, min_pts=5, want_points=False):
        """The same with the clouds in host memory (lk_clouds_mme): clouds float32 [n, 4] (x y z w records).  Returns the records, with want_points
        (records, n uint32, h float64, lmin float64), entry off[c] - off[0] + i for record off[c] + i."""
        c = np.ascontiguousarray(clouds, dtype=np.float32).reshape(-1, 4)
        if not want_points:
            return self._mme_call(self.L.lk_clouds_mme, _p(c), off, radius, min_pts, None, None, None)
        o = np.asarray(off, dtype=np.uint64)
        total = int(o[-1] - o[0]) if len(o) else 0
        cnt, hh, lm = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1)), np.zeros(max(total, 1))
        res = self._mme_call(self.L.lk_clouds_mme, _p(c), off, radius, min_pts, _p(cnt), _p(hh), _p(lm))
        return res, cnt[:total], hh[:total], lm[:total]

    def _sor_call(self, fn, clouds, off, k, reach, n_sigma, out_cloud, want_off, src_idx, keep, cnt, dbar):
        """What the two outlier-filter exports share - the offset tables and the records: fn(handle, clouds, table, k, reach, n_sigma, records,
        outputs).  Returns (records, out_off or None)."""
        o = np.ascontiguousarray(off, dtype=np.uint64)
        n = max(len(o) - 1, 0)
        res = np.zeros(max(n, 1), dtype=abi.sor_dtype())
        out_off = np.zeros(n + 1, dtype=np.uint64) if want_off else None
        self._chk(fn(self.h, clouds, n, _p(o), int(k), float(reach), float(n_sigma), _p(res), out_cloud, _p(out_off), src_idx, keep, cnt, dbar))
        return res[:n], out_off

    def clouds_sor_dev(self, d_clouds, off, k, reach, n_sigma, d_out=0, d_src_idx=0, d_keep=0, d_cnt=0, d_dbar=0, want_off=None):
        """Outliers removed from many clouds in device memory (lk_clouds_sor_dev): clouds_mme_dev's clouds and table.  A point with fewer than k
        (1 .. 32) other records within `reach` is isolated; the others get dbar, the mean distance to their k nearest, and are kept when dbar <=
        mu + n_sigma * sigma of their cloud (n_sigma = inf: the radius criterion alone).  d_out (device, room for off[-1] - off[0] records) takes
        the kept records in input order, cloud c at out_off[c] : out_off[c + 1]; d_src_idx their indices within their input clouds; d_keep uint8,
        d_cnt uint32, d_dbar float64 one entry per input record (0: none, each on its own).  Returns (abi.sor_dtype() records, out_off uint64 or
        None - given with d_out or d_src_idx, or when want_off is set); cloudmetrics.sor is the numpy statement."""
        want = bool(d_out or d_src_idx) if want_off is None else want_off
        return self._sor_call(self.L.lk_clouds_sor_dev, d_clouds, off, k, reach, n_sigma, d_out or None, want, d_src_idx or None, d_keep or None, d_cnt or None,
                              d_dbar or None)

    def clouds_sor(self, clouds, off, k, reach, n_sigma, want_points=False):
        """The same with the clouds in host memory (lk_clouds_sor): clouds float32 [n, 4] (x y z w records).  Returns (records, out_cloud float32
        [n_kept, 4], out_off uint64, src_idx uint32 [n_kept]), with want_points also (keep uint8, cnt uint32, dbar float64), entry
        off[c] - off[0] + i for record off[c] + i."""
        c = np.ascontiguousarray(clouds, dtype=np.float32).reshape(-1, 4)
        o = np.asarray(off, dtype=np.uint64)
        total = int(o[-1] - o[0]) if len(o) else 0
        out, src = np.zeros((max(total, 1), 4), dtype=np.float32), np.zeros(max(total, 1), dtype=np.uint32)
        keep, cnt, dbar = (np.zeros(max(total, 1), dtype=np.uint8), np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1))) if want_points else (None,) * 3
        res, out_off = self._sor_call(self.L.lk_clouds_sor, _p(c), off, k, reach, n_sigma, _p(out), True, _p(src), _p(keep), _p(cnt), _p(dbar))
        m = int(out_off[-1])
        if not want_points:
            return res, out[:m], out_off, src[:m]
        return res, out[:m], out_off, src[:m], keep[:total], cnt[:total], dbar[:total]

    def _cluster_call(self, fn, clouds, off, reach, min_pts, min_size, max_size, flags, label, kind, n_arr, cl_size, cl_first, want_cl_off, out_cloud, want_off, src_idx):
        """What the two clustering exports share - the offset tables and the records: fn(handle, clouds, table, reach, min_pts, the size bounds, flags,
        records, outputs).  Returns (records, cl_off or None, out_off or None)."""
        o = np.ascontiguousarray(off, dtype=np.uint64)
        n = max(len(o) - 1, 0)
        res = np.zeros(max(n, 1), dtype=abi.cluster_dtype())
        cl_off = np.zeros(n + 1, dtype=np.uint64) if want_cl_off else None
        out_off = np.zeros(n + 1, dtype=np.uint64) if want_off else None
        self._chk(fn(self.h, clouds, n, _p(o), float(reach), int(min_pts), int(min_size), int(max_size), int(flags), _p(res), label, kind, n_arr, cl_size, cl_first,
                     _p(cl_off), out_cloud, _p(out_off), src_idx))
        return res[:n], cl_off, out_off

    def clouds_cluster_dev(self, d_clouds, off, reach, min_pts=1, min_size=0, max_size=0xFFFFFFFF, flags=0, d_label=0, d_kind=0, d_n=0, d_cl_size=0, d_cl_first=0,
                           d_out=0, d_src_idx=0, want_cl_off=None, want_off=None):
        """Many clouds in device memory clustered (lk_clouds_cluster_dev, DBSCAN; min_pts = 1: the connected components within `reach`):
        clouds_mme_dev's clouds and table.  A point with at least min_pts records within `reach`, itself among them, is core; core points within
        reach of each other share a cluster; another point joins the cluster of its nearest core point within reach or is noise.  d_label uint32
        (the cluster's id within its cloud, 0xffffffff for noise), d_kind uint8 (0 noise, 1 border, 2 core), d_n uint32: one entry per input record;
        d_cl_size / d_cl_first uint32: cluster k of cloud c at entry cl_off[c] + k; d_out / d_src_idx: the points of the clusters with min_size <=
        size <= max_size (flags = abi.LK_CLUSTER_KEEP_LARGEST: of the largest of them) in input order, cloud c at out_off[c] : out_off[c + 1]
        (0: none, each on its own).  Returns (abi.cluster_dtype() records, cl_off uint64 or None, out_off uint64 or None) - a table is given with
        the arrays that need it, or when its want_ is set; cloudmetrics.cluster is the numpy statement."""
        wc = bool(d_cl_size or d_cl_first) if want_cl_off is None else want_cl_off
        wo = bool(d_out or d_src_idx) if want_off is None else want_off
        return self._cluster_call(self.L.lk_clouds_cluster_dev, d_clouds, off, reach, min_pts, min_size, max_size, flags, d_label or None, d_kind or None, d_n or None,
                                  d_cl_size or None, d_cl_first or None, wc, d_out or None, wo, d_src_idx or None)

    def clouds_cluster(self, clouds, off, reach, min_pts=1, min_size=0, max_size=0xFFFFFFFF, flags=0):
        """The same with the clouds in host memory (lk_clouds_cluster): clouds float32 [n, 4] (x y z w records).  Returns a dict: res (records), label
        uint32, kind uint8, n uint32 (entry off[c] - off[0] + i for record off[c] + i), cl_size, cl_first uint32 and cl_off uint64, out float32
        [n_kept, 4], out_off uint64, src_idx uint32 [n_kept]."""
        c = np.ascontiguousarray(clouds, dtype=np.float32).reshape(-1, 4)
        o = np.asarray(off, dtype=np.uint64)
        total = int(o[-1] - o[0]) if len(o) else 0
        u32 = lambda: np.zeros(max(total, 1), dtype=np.uint32)   # noqa: E731
        label, kind, n_arr, cl_size, cl_first, src = u32(), np.zeros(max(total, 1), dtype=np.uint8), u32(), u32(), u32(), u32()
        out = np.zeros((max(total, 1), 4), dtype=np.float32)
        res, cl_off, out_off = self._cluster_call(self.L.lk_clouds_cluster, _p(c), off, reach, min_pts, min_size, max_size, flags, _p(label), _p(kind), _p(n_arr),
                                                  _p(cl_size), _p(cl_first), True, _p(out), True, _p(src))
        k, m = int(cl_off[-1]), int(out_off[-1])
        return dict(res=res, label=label[:total], kind=kind[:total], n=n_arr[:total], cl_size=cl_size[:k], cl_first=cl_first[:k], cl_off=cl_off, out=out[:m],
                    out_off=out_off, src_idx=src[:m])

    def _planes_call(self, fn, clouds, off, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, label, out_cloud, want_off, src_idx):
        """What the two plane-extraction exports share - the offset tables and the records: fn(handle, clouds, table, the RANSAC's arguments, records,
        outputs).  Returns (per-cloud records, per-plane records [n_clouds, max_planes], out_off or None)."""
        o = np.ascontiguousarray(off, dtype=np.uint64)
        n = max(len(o) - 1, 0)
        res = np.zeros(max(n, 1), dtype=abi.planes_dtype())
        pl = np.zeros((max(n, 1), max(int(max_planes), 1)), dtype=abi.plane_dtype())
        ax = None if axis is None else np.ascontiguousarray(axis, dtype=np.float64).reshape(3)
        out_off = np.zeros(n + 1, dtype=np.uint64) if want_off else None
        self._chk(fn(self.h, clouds, n, _p(o), float(dist), int(n_hyp), int(max_planes), int(min_inliers), _p(ax), float(cos_max_angle), int(seed), int(flags),
                     _p(res), _p(pl), label, out_cloud, _p(out_off), src_idx))
        return res[:n], pl[:n], out_off

    def clouds_planes_dev(self, d_clouds, off, dist, n_hyp=256, max_planes=4, min_inliers=100, axis=None, cos_max_angle=0.0, seed=0, flags=0, d_label=0, d_out=0,
                          d_src_idx=0, want_off=None):
        """Dominant planes peeled off many clouds in device memory (lk_clouds_planes_dev, RANSAC): clouds_mme_dev's clouds and table.  Per round n_hyp
        planes through three sampled records of what is left; the one with the most records within `dist` wins (the smallest number among equals), its
        records become plane r, up to max_planes rounds while a winner holds min_inliers.  axis (3 floats) with cos_max_angle keeps the planes whose
        normal lies within that angle of the axis.  d_label uint32 per input record (the plane's number, 0xffffffff: none); d_out / d_src_idx: the
        remainder (flags = abi.LK_PLANES_KEEP_PLANES: the points on planes) in input order, cloud c at out_off[c] : out_off[c + 1] (0: none, each on
        its own).  Returns (abi.planes_dtype() records, abi.plane_dtype() records [n_clouds, max_planes], out_off uint64 or None);
        cloudmetrics.planes is the numpy statement."""
        wo = bool(d_out or d_src_idx) if want_off is None else want_off
        return self._planes_call(self.L.lk_clouds_planes_dev, d_clouds, off, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, d_label or None,
                                 d_out or None, wo, d_src_idx or None)

    def clouds_planes(self, clouds, off, dist, n_hyp=256, max_planes=4, min_inliers=100, axis=None, cos_max_angle=0.0, seed=0, flags=0):
        """The same with the clouds in host memory (lk_clouds_planes): clouds float32 [n, 4] (x y z w records).  Returns a dict: res (per-cloud
        records), planes (per-plane records [n_clouds, max_planes]), label uint32 (entry off[c] - off[0] + i for record off[c] + i), out float32
        [n_kept, 4], out_off uint64, src_idx uint32 [n_kept]."""
        c = np.ascontiguousarray(clouds, dtype=np.float32).reshape(-1, 4)
        o = np.asarray(off, dtype=np.uint64)
        total = int(o[-1] - o[0]) if len(o) else 0
        label, src = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.uint32)
        out = np.zeros((max(total, 1), 4), dtype=np.float32)
        res, pl, out_off = self._planes_call(self.L.lk_clouds_planes, _p(c), off, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, _p(label),
                                             _p(out), True, _p(src))
        m = int(out_off[-1])
        return dict(res=res, planes=pl, label=label[:total], out=out[:m], out_off=out_off, src_idx=src[:m])

    def downsample_clouds_dev(self, d_world, file_off, leaf, d_out):
        """Downsampled map clouds of many files in one call (lk_downsample_clouds_dev): file f = the 16-byte x y z intensity records
        file_off[f] : file_off[f + 1] at the device pointer d_world (a run replay's d_world_out; pcd_file_offsets gives the table), pcl::VoxelGrid at
        `leaf` per file -> d_out (device, room for file_off[-1] - file_off[0] records).  Returns (out_off uint64 [n_files + 1], unfiltered uint8
        [n_files]): file f's cloud is d_out[out_off[f] : out_off[f + 1]]; unfiltered[f] = 1 where the grid would overflow and the file is its input."""
        fo = np.ascontiguousarray(file_off, dtype=np.uint64)
        n_files = max(len(fo) - 1, 0)
        out_off = np.zeros(n_files + 1, dtype=np.uint64)
        unf = np.zeros(max(n_files, 1), dtype=np.uint8)
        self._chk(self.L.lk_downsample_clouds_dev(self.h, d_world, n_files, _p(fo), leaf, d_out, _p(out_off), _p(unf)))
        return out_off, unf[:n_files]

    def downsample_clouds(self, world, file_off, leaf, with_flags=False):
        """The same from host memory (lk_downsample_clouds): world float32 [n, 4] -> a list of (n_f, 4) float32 arrays, one per file; with_flags:
        (that list, unfiltered)."""
        w = np.ascontiguousarray(world, dtype=np.float32)
        fo = np.ascontiguousarray(file_off, dtype=np.uint64)
        n_files = len(fo) - 1
        out = np.zeros((int(fo[-1] - fo[0]), 4), dtype=np.float32)
        out_off = np.zeros(n_files + 1, dtype=np.uint64)
        unf = np.zeros(n_files, dtype=np.uint8)
        self._chk(self.L.lk_downsample_clouds(self.h, _p(w), n_files, _p(fo), leaf, _p(out), _p(out_off), _p(unf)))
        clouds = [out[int(a):int(b)].copy() for a, b in zip(out_off[:-1], out_off[1:])]
        return (clouds, unf) if with_flags else clouds

    def _map_clouds_staged(self, d_world, run_off, scan_off, frames_per_file, leaf):
        """d_world_out of a run replay -> the map files' downsampled clouds, on the device but for the result: a dict with "clouds" (a list of (n_f, 4)
        float32 arrays), "file_off", "file_run", "unfiltered"."""
        file_off, file_run = pcd_file_offsets(run_off, scan_off, frames_per_file)
        res = dict(clouds=[], file_off=file_off, file_run=file_run, unfiltered=np.zeros(0, dtype=np.uint8))
        if len(file_run) == 0:
            return res
        n = int(file_off[-1] - file_off[0])
        with self._staged(16 * n) as (d_out,):
            out_off, res["unfiltered"] = self.downsample_clouds_dev(d_world, file_off, leaf, d_out)
            out = np.zeros((int(out_off[-1]), 4), dtype=np.float32)
            if len(out):
                self.d2h(out, d_out)
        res["clouds"] = [out[int(a):int(b)].copy() for a, b in zip(out_off[:-1], out_off[1:])]
        return res

    def _replay_runs_staged(self, entry, runs, t_begins, xs, Ps, imus, kins, cloud=False, bucket_poses=False, map_clouds=None, **kw):
        """What the two run conveniences share: priors, flatten_runs, points and messages -> HBM, entry(...), the poses run by run.  cloud /
        bucket_poses / map_clouds: `entry` is the _cloud form; returns (poses run by run, dict) with "cloud" (float32 [n, 4], in the order of the
        flattened points) and / or "bucket_poses" (all records) + "scan_bucket_off" and / or "map_clouds" (map_clouds = (frames_per_file, leaf):
        _map_clouds_staged on the registered cloud while it is in HBM)."""
        if xs is not None:
            self.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        t = flatten_runs(runs, t_begins, imus, kins)
        world_bytes = 16 * len(t["pts"]) if cloud or map_clouds is not None else None
        with self._staged(t["pts"], t["msgs"], world_bytes) as (d_pts, d_msgs, d_world):
            extra = None
            if cloud or bucket_poses or map_clouds is not None:
                extra = {}
                poses, sbo = entry(d_pts, t["run_off"], t["scan_off"], t["t_begin"], t["msg_kind"], t["n_msg"], d_msgs, d_world=d_world, **kw)
                if cloud:
                    extra["cloud"] = np.zeros((len(t["pts"]), 4), dtype=np.float32)
                    self.d2h(extra["cloud"], d_world)
                if bucket_poses:
                    extra["bucket_poses"], extra["scan_bucket_off"] = self.runs_bucket_poses(0, int(sbo[-1])), sbo
                if map_clouds is not None:
                    extra["map_clouds"] = self._map_clouds_staged(d_world, t["run_off"], t["scan_off"], *map_clouds)
            else:
                poses = entry(d_pts, t["run_off"], t["scan_off"], t["t_begin"], t["msg_kind"], t["n_msg"], d_msgs, **kw)
            by_run = [poses[int(a):int(b)] for a, b in zip(t["run_off"][:-1], t["run_off"][1:])]
            return by_run if extra is None else (by_run, extra)

    def batch_replay_overlay_runs(self, runs, t_begins, xs=None, Ps=None, imus=None, kins=None, cloud=False, bucket_poses=False, map_clouds=None):
        """Convenience: runs = a list of runs, each a list of host scans (lk_point arrays, time-sorted, any sizes); t_begins, imus / kins: the same
        nesting (one start time, one message array per scan) -> HBM -> batch_replay_overlay_runs_dev.  Optional priors, one per run.  Returns the
        poses run by run (a list of lists); with cloud / bucket_poses: (those, dict) - the registered cloud and / or the bucket table of
        batch_replay_overlay_runs_cloud_dev (_replay_runs_staged); map_clouds = (frames_per_file, leaf): also the map files' downsampled clouds
        (pcd_file_offsets + downsample_clouds_dev on the registered cloud, chained on the device) under "map_clouds"."""
        if cloud or bucket_poses or map_clouds is not None:
            return self._replay_runs_staged(self.batch_replay_overlay_runs_cloud_dev, runs, t_begins, xs, Ps, imus, kins, cloud=cloud, bucket_poses=bucket_poses,
                                            map_clouds=map_clouds)
        return self._replay_runs_staged(self.batch_replay_overlay_runs_dev, runs, t_begins, xs, Ps, imus, kins)

    def batch_replay_runs_dev(self, d_pts, run_off, scan_off, t_begins, msg_kind=0, n_msg=None, d_msgs=0, cont=False, want_poses=True, flags=None):
        """Whole recorded runs on the FROZEN map, run r on slot r (lk_batch_replay_runs_dev): arguments as for batch_replay_overlay_runs_dev; no insert,
        the handle's map is unchanged.  State, covariance and both time stamps of a slot survive its run's scan boundaries.  cont: LK_RUNS_CONTINUE -
        the slots go on from what they hold (the caller has not used them since the previous call), so a run may be fed in chunks of scans.
        Returns one pose per SCAN (counters of that scan alone); batch_get_states gives the runs' final states."""
        fl = (LK_RUNS_CONTINUE if cont else 0) if flags is None else int(flags)
        return self._runs_call(self.L.lk_batch_replay_runs_dev, d_pts, run_off, scan_off, t_begins, msg_kind, n_msg, d_msgs, want_poses, (fl,))

    def batch_replay_runs(self, runs, t_begins, xs=None, Ps=None, imus=None, kins=None, cont=False, cloud=False, bucket_poses=False, map_clouds=None):
        """Convenience: the nested host inputs of batch_replay_overlay_runs -> HBM -> batch_replay_runs_dev (frozen map).  Optional priors, one per
        run (not with cont: a continued run goes on from what its slot holds).  Returns the poses run by run (a list of lists); with cloud /
        bucket_poses / map_clouds: (those, dict), as batch_replay_overlay_runs."""
        assert not (cont and xs is not None), "a continued run keeps its slot's state: no priors"
        if cloud or bucket_poses or map_clouds is not None:
            return self._replay_runs_staged(self.batch_replay_runs_cloud_dev, runs, t_begins, xs, Ps, imus, kins, cloud=cloud, bucket_poses=bucket_poses,
                                            map_clouds=map_clouds, cont=cont)
        return self._replay_runs_staged(self.batch_replay_runs_dev, runs, t_begins, xs, Ps, imus, kins, cont=cont)

    def overlay_reserve(self, roots_per_scan=0, nodes_per_scan=0, blocks_per_scan=0):
        self._chk(self.L.lk_overlay_reserve(self.h, roots_per_scan, nodes_per_scan, blocks_per_scan))

    def overlay_export(self, slot):
        """Map blob of the voxels scan `slot` of the last overlay replay holds privately."""
        return self._export_blob(self.L.lk_overlay_export, self.h, slot)

    def overlay_commit(self, slot, adopt_filter=False, flags=None):
        """Slot `slot`'s overlay of the last replay with insert becomes part of the handle's map, on the device (lk_overlay_commit): the map
        KILO::process of that slot's scans would have left on a private copy.  The replay's overlays are stale afterwards.  adopt_filter: the slot's
        filter record (state, covariance, time stamps, counters) is also copied to slot 0.  flags: the raw flag word instead."""
        fl = (abi.LK_COMMIT_ADOPT_FILTER if adopt_filter else 0) if flags is None else int(flags)
        self._chk(self.L.lk_overlay_commit(self.h, slot, fl))

    def overlay_stats(self):
        """(max roots, max nodes, max point blocks) any scan's overlay reached in the last overlay replay."""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.lk_overlay_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def overlay_resident_rounds(self):
        """Launches of the scan-resident kernel in the last recorded-run replay with insert (0: it ran launch by launch)."""
        r = C.c_uint32(0)
        self._chk(self.L.lk_overlay_resident_rounds(self.h, C.byref(r)))
        return int(r.value)

    def overlay_pool_bytes(self):
        """(bytes the overlay pools hold, per-scan root-table entries, child nodes, point blocks)."""
        n, a, b, c = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.lk_overlay_pool_bytes(self.h, C.byref(n), C.byref(a), C.byref(b), C.byref(c)))
        return n.value, a.value, b.value, c.value

    @staticmethod
    def ragged_tables(scan_off, bucket_offs, bucket_dts, t_begins, imus=None, kins=None):
        """Flatten per-scan bucket tables into the arrays lk_batch_replay_ragged_dev takes (do this once per recorded run,
        not per replay): scan s = points [scan_off[s], scan_off[s+1]) with bucket bounds bucket_offs[s] (n_b + 1 offsets
        relative to the scan), time offsets bucket_dts[s] (n_b) and start time t_begins[s]."""
        n_scans = len(bucket_dts)
        so = np.ascontiguousarray(scan_off, dtype=np.uint64)
        assert len(so) == n_scans + 1 and len(bucket_offs) == n_scans and len(t_begins) == n_scans
        nb = np.fromiter((len(d) for d in bucket_dts), dtype=np.uint32, count=n_scans)
        off = np.ascontiguousarray(np.concatenate(bucket_offs), dtype=np.uint32)
        dt = np.ascontiguousarray(np.concatenate(bucket_dts), dtype=np.float64)
        assert len(off) == int(nb.sum()) + n_scans and len(dt) == int(nb.sum())
        tab = dict(n_scans=n_scans, scan_off=so, n_buckets=nb, bucket_off=off, bucket_dt=dt, t_begin=_f64(t_begins))
        if imus is not None:   # per-scan lk_imu arrays (stamp, acc, gyr), time-sorted: applied between the buckets (KILO.cc:379-383)
            assert len(imus) == n_scans
            tab["n_imu"] = np.fromiter((len(m) for m in imus), dtype=np.uint32, count=n_scans)
            tab["imus"] = np.ascontiguousarray(np.concatenate([np.asarray(m) for m in imus])) if tab["n_imu"].sum() else np.zeros(0, dtype=np.float64)
            assert tab["imus"].nbytes == 56 * int(tab["n_imu"].sum())
        if kins is not None:   # per-scan lk_kin_imu arrays (leg-fusion mode, KILO.cc:384-390)
            assert len(kins) == n_scans and imus is None
            tab["n_kin"] = np.fromiter((len(m) for m in kins), dtype=np.uint32, count=n_scans)
            tab["kins"] = np.ascontiguousarray(np.concatenate([np.asarray(m) for m in kins])) if tab["n_kin"].sum() else np.zeros(0, dtype=np.float64)
            assert tab["kins"].nbytes == 264 * int(tab["n_kin"].sum())
        return tab

    @staticmethod
    def _ragged_messages(t):
        """(msg_kind, n_msg, records) of a ragged_tables() dict: its kins (2), its imus (1), or (0, None, None)."""
        return (2, t["n_kin"], t["kins"]) if "n_kin" in t else (1, t["n_imu"], t["imus"]) if "n_imu" in t else (0, None, None)

    def batch_replay_ragged_dev(self, d_pts, tables, want_poses=True):
        """Ragged batch on slots [0, n_scans): `tables` from ragged_tables()."""
        t = tables
        n_scans = t["n_scans"]
        poses = (abi.lk_pose * n_scans)() if want_poses else None
        kind, n_msg, msgs = self._ragged_messages(t)
        fn = (self.L.lk_batch_replay_ragged_dev, self.L.lk_batch_replay_ragged_imu_dev, self.L.lk_batch_replay_ragged_kin_dev)[kind]
        self._chk(fn(self.h, d_pts, n_scans, _p(t["scan_off"]), _p(t["n_buckets"]), _p(t["bucket_off"]), _p(t["bucket_dt"]), _p(t["t_begin"]),
                     *((_p(n_msg), _p(msgs)) if kind else ()), poses))
        return poses

    def batch_replay_scans_dev(self, d_pts, scan_off, t_begins, imus=None, kins=None, want_poses=True):
        """Ragged batch on slots [0, n_scans) with the bucket tables built ON THE DEVICE (lk_batch_replay_scans_dev): the host
        passes the scans' offsets and start times only.  imus / kins: per-scan message arrays (or None)."""
        so = np.ascontiguousarray(scan_off, dtype=np.uint64)
        n_scans = len(so) - 1
        tb = _f64(t_begins)
        assert len(tb) == n_scans
        kind, n_msg, flat = _messages(imus, kins, n_scans)   # flat None when no scan has a message: the entry asks for the array only if one has
        poses = (abi.lk_pose * n_scans)() if want_poses else None
        self._chk(self.L.lk_batch_replay_scans_dev(self.h, d_pts, n_scans, _p(so), _p(tb), kind, _p(n_msg), _p(flat), poses))
        return poses

    def batch_replay_ragged(self, scans, t_begins, xs=None, Ps=None, imus=None, kins=None, host_tables=False):
        """Convenience: host scans (lists of lk_point arrays, time-sorted) -> HBM, buckets = runs of equal curvature
        (KILO.cc:375-378), optional priors, ragged replay.  Returns the poses.  The bucket tables are built on the device
        (lk_batch_replay_scans_dev); host_tables=True builds them here and goes through lk_batch_replay_ragged(_imu/_kin)_dev
        (same results, bit for bit)."""
        if xs is not None:
            self.batch_set_priors(np.asarray(xs), np.asarray(Ps))
        allpts = np.ascontiguousarray(np.concatenate(scans))
        scan_off = np.r_[0, np.cumsum([len(sc) for sc in scans])]
        with self._staged(allpts) as (d,):
            if not host_tables:
                return self.batch_replay_scans_dev(d, scan_off, t_begins, imus=imus, kins=kins)
            tabs = [synth.buckets_of(sc) for sc in scans]
            return self.batch_replay_ragged_dev(d, self.ragged_tables(scan_off, [t[0] for t in tabs], [t[1] for t in tabs], t_begins, imus, kins))

    # ---- leg kinematics front end (HighState -> lk_kin_imu, the kin branch of syncPackage) ----
    def kin_configure(self, params=None):
        """Kinematics::Config + `redundancy` from a yaml-keyed parameter dict (config.kin_config); resets the carried state."""
        from . import config

        self._chk(self.L.lk_kin_configure(self.h, C.byref(config.kin_config(params))))

    def kin_get_frontend(self):
        """The carried state as a dict(contact int32[4], last_acc_z, last_gyr_z, last_stamp)."""
        st = abi.lk_kin_frontend_state()
        self._chk(self.L.lk_kin_get_frontend(self.h, C.byref(st)))
        return dict(contact=np.array(st.contact, dtype=np.int32), last_acc_z=np.float32(st.last_acc_z), last_gyr_z=np.float32(st.last_gyr_z),
                    last_stamp=st.last_stamp)

    def kin_set_frontend(self, fe):
        st = abi.lk_kin_frontend_state()
        st.contact = (C.c_int32 * 4)(*[int(v) for v in fe["contact"]])
        st.last_acc_z, st.last_gyr_z, st.last_stamp = float(fe["last_acc_z"]), float(fe["last_gyr_z"]), float(fe["last_stamp"])
        self._chk(self.L.lk_kin_set_frontend(self.h, C.byref(st)))

    def decode_highstate(self, msgs):
        """Serialized HighState messages (bytes / uint8 array, n x LK_HIGHSTATE_BYTES) -> KIN_DTYPE records of the kept ones."""
        data = np.ascontiguousarray(np.frombuffer(bytes(msgs) if not isinstance(msgs, np.ndarray) else msgs.tobytes(), dtype=np.uint8))
        assert data.size % abi.LK_HIGHSTATE_BYTES == 0
        n = data.size // abi.LK_HIGHSTATE_BYTES
        out = np.zeros(max(n, 1), dtype=synth.KIN_DTYPE)
        n_out = C.c_size_t(0)
        self._chk(self.L.lk_decode_highstate(self.h, _p(data), n, _p(out), C.byref(n_out)))
        return out[: n_out.value]

    def decode_highstate_dev(self, d_msgs, n, d_out):
        """n messages in HBM -> records at the device pointer d_out (room for n); returns the number kept."""
        n_out = C.c_size_t(0)
        self._chk(self.L.lk_decode_highstate_dev(self.h, d_msgs, n, d_out, C.byref(n_out)))
        return n_out.value

    def kin_split_dev(self, d_kins, n_kins, scan_end):
        """syncPackage's kin branch over n_kins time-sorted records in HBM and the scans' end times -> (n_msg uint32[n_scans], n_packaged,
        n_consumed)."""
        return self._split_dev(self.L.lk_kin_split_dev, d_kins, n_kins, scan_end)

    def _split_dev(self, fn, d_msgs, n, scan_end):
        """The body of kin_split_dev / imu_split_dev: fn = the export of the record kind at d_msgs."""
        ends = _f64(scan_end)
        n_msg = np.zeros(max(len(ends), 1), dtype=np.uint32)
        npk, ncs = C.c_size_t(0), C.c_size_t(0)
        self._chk(fn(self.h, d_msgs, n, _p(ends), len(ends), _p(n_msg), C.byref(npk), C.byref(ncs)))
        return n_msg[: len(ends)], npk.value, ncs.value

    def batch_replay_scans_kin_dev(self, d_pts, scan_off, t_begins, n_msg, d_kins, want_poses=True):
        """lk_batch_replay_scans_dev in leg-fusion mode with the records already in HBM (d_kins: n_msg[s] records per scan, concatenated)."""
        return self._replay_scans_msgs_dev(self.L.lk_batch_replay_scans_kin_dev, d_pts, scan_off, t_begins, n_msg, d_kins, want_poses)

    def _replay_scans_msgs_dev(self, fn, d_pts, scan_off, t_begins, n_msg, d_msgs, want_poses):
        """The body of batch_replay_scans_kin_dev / _imu_dev: fn = the export of the record kind at d_msgs."""
        so = np.ascontiguousarray(scan_off, dtype=np.uint64)
        n_scans = len(so) - 1
        tb = _f64(t_begins)
        nm = np.ascontiguousarray(n_msg, dtype=np.uint32)
        assert len(tb) == n_scans and len(nm) == n_scans
        poses = (abi.lk_pose * n_scans)() if want_poses else None
        self._chk(fn(self.h, d_pts, n_scans, _p(so), _p(tb), _p(nm), d_msgs, poses))
        return poses

    # ---- IMU front end (sensor_msgs/Imu -> lk_imu, the IMU branch of syncPackage) ----
    def imu_configure(self, redundancy=True):
        """Sets the yaml key `redundancy` (a bool, or a parameter dict holding it) and resets the carried state."""
        if isinstance(redundancy, dict):
            redundancy = redundancy.get("redundancy", True)
        self._chk(self.L.lk_imu_configure(self.h, 1 if redundancy else 0))

    def imu_get_frontend(self):
        """The carried state as a dict(last_acc_z, last_gyr_z, last_stamp)."""
        st = abi.lk_imu_frontend_state()
        self._chk(self.L.lk_imu_get_frontend(self.h, C.byref(st)))
        return dict(last_acc_z=st.last_acc_z, last_gyr_z=st.last_gyr_z, last_stamp=st.last_stamp)

    def imu_set_frontend(self, fe):
        st = abi.lk_imu_frontend_state(float(fe["last_acc_z"]), float(fe["last_gyr_z"]), float(fe["last_stamp"]))
        self._chk(self.L.lk_imu_set_frontend(self.h, C.byref(st)))

    def decode_imu(self, buf, msg_off):
        """Serialized sensor_msgs/Imu messages (uint8 array; message i = buf[msg_off[i]:msg_off[i + 1]]) -> IMU_DTYPE records of the kept ones."""
        data = np.ascontiguousarray(buf, dtype=np.uint8)
        mo = np.ascontiguousarray(msg_off, dtype=np.uint64)
        n = len(mo) - 1
        out = np.zeros(max(n, 1), dtype=synth.IMU_DTYPE)
        n_out = C.c_size_t(0)
        self._chk(self.L.lk_decode_imu(self.h, _p(data), n, _p(mo), _p(out), C.byref(n_out)))
        return out[: n_out.value]

    def decode_imu_dev(self, d_msgs, msg_off, d_out):
        """len(msg_off) - 1 messages in HBM (message i at d_msgs + msg_off[i]) -> records at the device pointer d_out (room for one per
        message); returns the number kept."""
        mo = np.ascontiguousarray(msg_off, dtype=np.uint64)
        n_out = C.c_size_t(0)
        self._chk(self.L.lk_decode_imu_dev(self.h, d_msgs, len(mo) - 1, _p(mo), d_out, C.byref(n_out)))
        return n_out.value

    def imu_split_dev(self, d_imus, n_imus, scan_end):
        """syncPackage's IMU branch over n_imus time-sorted lk_imu records in HBM and the scans' end times -> (n_msg uint32[n_scans],
        n_packaged, n_consumed)."""
        return self._split_dev(self.L.lk_imu_split_dev, d_imus, n_imus, scan_end)

    def batch_replay_scans_imu_dev(self, d_pts, scan_off, t_begins, n_msg, d_imus, want_poses=True):
        """lk_batch_replay_scans_dev in IMU-only mode with the records already in HBM (d_imus: n_msg[s] records per scan, concatenated)."""
        return self._replay_scans_msgs_dev(self.L.lk_batch_replay_scans_imu_dev, d_pts, scan_off, t_begins, n_msg, d_imus, want_poses)

    # ---- first frame (KILO.cc:332-352) ----
    def first_frame(self, raw_pts, end_time, imus=None, kins=None):
        """State initialisation from the first package's messages (imus: IMU_DTYPE, or kins: KIN_DTYPE), cloudLidarToWorld on the RAW first
        cloud, BuildVoxelMap, acc_norm and the time stamps, on slot 0 (lk_first_frame)."""
        assert (imus is None) != (kins is None)
        raw = np.ascontiguousarray(raw_pts)
        msgs = np.ascontiguousarray(imus if kins is None else kins)
        self._chk(self.L.lk_first_frame(self.h, _p(raw), len(raw), end_time, 1 if kins is None else 2, _p(msgs), len(msgs)))

    def first_frame_dev(self, d_raw, n, end_time, msg_kind, d_msgs, n_msg):
        """The same with the raw cloud (n lk_point) and the n_msg records (msg_kind 1: lk_imu, 2: lk_kin_imu) already in HBM."""
        self._chk(self.L.lk_first_frame_dev(self.h, d_raw, n, end_time, msg_kind, d_msgs, n_msg))

    # ---- measurement / memory hooks ----
    def profile_enable(self, on):
        self._chk(self.L.lk_profile_enable(self.h, int(on)))

    def profile_get(self, name):
        n, ms = C.c_uint64(), C.c_double()
        self._chk(self.L.lk_profile_get(self.h, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_reset(self):
        self._chk(self.L.lk_profile_reset(self.h))

    def device_malloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.L.lk_device_malloc(self.h, C.byref(p), nbytes))
        return p.value

    def device_free(self, ptr):
        self._chk(self.L.lk_device_free(self.h, ptr))

    def h2d(self, d_ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.lk_memcpy_h2d(self.h, d_ptr, _p(arr), arr.nbytes))

    def d2h(self, arr, d_ptr):
        assert arr.flags["C_CONTIGUOUS"]
        self._chk(self.L.lk_memcpy_d2h(self.h, _p(arr), d_ptr, arr.nbytes))

    def synchronize(self):
        self._chk(self.L.lk_synchronize(self.h))

    def stream(self):
        return self.L.lk_stream(self.h)

    def stream_pipeline(self, on):
        """Pipelined stream path on / off (lk_stream_pipeline)."""
        self._chk(self.L.lk_stream_pipeline(self.h, 1 if on else 0))

    def stream_resident(self, on):
        """Scan-resident stream kernel on / off (lk_stream_resident)."""
        self._chk(self.L.lk_stream_resident(self.h, 1 if on else 0))

    def stream_grid(self, mode):
        """Grid-resident stream kernel for scans of large buckets (lk_stream_grid): 0 / False never, 1 / True buckets up to 4096 points, 2 any size."""
        self._chk(self.L.lk_stream_grid(self.h, int(mode)))

    def stream_grid_placement(self):
        """Bit mask of the XCC ids the working blocks of the last one-XCD grid-resident launch ran on (lk_stream_grid_placement)."""
        m = C.c_uint32(0)
        self._chk(self.L.lk_stream_grid_placement(self.h, C.byref(m)))
        return int(m.value)

    def test_stall(self, bound_ms):
        """Fault injection for the LK_ERR_TIMEOUT path of the resident stream kernels (include/legkilo_hip.h: lk_test_stall); 0 = off."""
        self._chk(self.L.lk_test_stall(self.h, int(bound_ms)))

    def stream_resident_stats(self):
        """(scans through the scan-resident kernel, launches beyond one per scan: its fallback rounds)."""
        out = np.zeros(2, dtype=np.uint64)
        self._chk(self.L.lk_stream_resident_stats(self.h, _p(out)))
        return int(out[0]), int(out[1])

    def stream_resident_redo(self):
        """Buckets the scan-resident kernel's filter wave evaluated again after a conflicting insert (lk_stream_stats' fourth word)."""
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.L.lk_stream_stats(self.h, _p(out)))
        return int(out[3])

    def stream_stats(self):
        """(pipelined buckets, their residual tiles, tiles the verify pass evaluated again)."""
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.L.lk_stream_stats(self.h, _p(out)))
        return int(out[0]), int(out[1]), int(out[2])
