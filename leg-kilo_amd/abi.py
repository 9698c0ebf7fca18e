"""ctypes mirrors of the PODs in include/legkilo_hip.h (keep field order identical) and the C signatures of its prototypes."""
import ctypes as C
import functools
import os
import re

LK_DIM_STATE = 30
LK_STATE_DOUBLES = 36
LK_BLOCK_PTS = 52
LK_BLOB_MAGIC = 0x4C4B4D50

LK_PLANE_IS_PLANE = 1
LK_PLANE_IS_INIT = 2
LK_NODE_INIT_OCTO = 1
LK_NODE_UPDATE_ENABLE = 2
LK_NODE_OCTO_STATE = 4
LK_NODE_PTS_DROPPED = 8

LK_COMMIT_ADOPT_FILTER = 1   # lk_overlay_commit: the committed slot's filter record also goes to slot 0


class LegKiloError(RuntimeError):
    pass


_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "legkilo_hip.h")
_PROTOTYPE = re.compile(r"^([A-Za-z_][\w \*]*?)\b(lk_\w+)\s*\(([^;{]*?)\)\s*;", re.M)
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "unsigned int": C.c_uint32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float}


def _ctype(decl, name, is_return=False):
    """The ctypes type of one C type as the header writes it; `name`: the prototype, for the error."""
    t = " ".join(decl.replace("*", " * ").split())
    if t.endswith("*"):
        return C.c_char_p if t == "const char *" else C.c_void_p
    if is_return and t == "void":
        return None
    if t not in _SCALARS:
        raise LegKiloError(f"include/legkilo_hip.h: {name}: no ctypes type for {'return type' if is_return else 'parameter'} '{decl.strip()}'")
    return _SCALARS[t]


def parse_signatures(header_text):
    """{name: (restype, [argtypes])} of every lk_* prototype in the text of a header.  Nothing is guessed: a type outside the closed map
    of _ctype, or an `lk_*(` that is not a prototype this reads, raises a LegKiloError that names it."""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        params = [p.strip() for p in params.split(",")] if params.strip() != "void" else []
        sigs[name] = (_ctype(ret, name, True), [_ctype(re.sub(r"\w+$", "", p), name) for p in params])   # a parameter = its type, then its name
    unread = sorted(set(re.findall(r"\b(lk_\w+)\s*\(", text)) - set(sigs))
    if unread:
        raise LegKiloError(f"include/legkilo_hip.h: cannot read the prototype of {', '.join(unread)}")
    return sigs


@functools.lru_cache(maxsize=None)
def signatures():
    """parse_signatures of include/legkilo_hip.h: what binding.lib() sets as restype / argtypes, and binding.EXPORTS."""
    with open(_HEADER) as f:
        return parse_signatures(f.read())


class lk_config(C.Structure):
    _fields_ = [
        ("vel_process_cov", C.c_double),
        ("imu_acc_process_cov", C.c_double),
        ("imu_gyr_process_cov", C.c_double),
        ("contact_process_cov", C.c_double),
        ("acc_bias_process_cov", C.c_double),
        ("gyr_bias_process_cov", C.c_double),
        ("kin_bias_process_cov", C.c_double),
        ("imu_acc_meas_noise", C.c_double),
        ("imu_acc_z_meas_noise", C.c_double),
        ("imu_gyr_meas_noise", C.c_double),
        ("kin_meas_noise", C.c_double),
        ("chd_meas_noise", C.c_double),
        ("contact_meas_noise", C.c_double),
        ("lidar_point_meas_ratio", C.c_double),
        ("max_voxel_size", C.c_double),
        ("planner_threshold", C.c_double),
        ("beam_err", C.c_double),
        ("dept_err", C.c_double),
        ("sigma_num", C.c_double),
        ("max_layer", C.c_int32),
        ("max_iterations", C.c_int32),
        ("layer_init_num", C.c_int32 * 5),
        ("max_points_num", C.c_int32),
        ("ext_R", C.c_double * 9),
        ("ext_T", C.c_double * 3),
        ("gravity", C.c_double),
        ("device_id", C.c_int32),
        ("n_slots", C.c_uint32),
        ("max_roots", C.c_uint32),
        ("max_nodes", C.c_uint32),
        ("max_point_blocks", C.c_uint32),
        ("max_scan_points", C.c_uint32),
    ]


class lk_point(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("curvature", C.c_float)]


class lk_imu(C.Structure):
    _fields_ = [("stamp", C.c_double), ("acc", C.c_double * 3), ("gyr", C.c_double * 3)]


class lk_kin_imu(C.Structure):
    _fields_ = [
        ("time_stamp", C.c_double),
        ("foot_pos", (C.c_double * 3) * 4),
        ("foot_vel", (C.c_double * 3) * 4),
        ("contact", C.c_int32 * 4),
        ("acc", C.c_double * 3),
        ("gyr", C.c_double * 3),
    ]


LK_HIGHSTATE_BYTES = 1095   # ROS1 serialisation of unitree_legged_msgs/HighState (fixed size)


class lk_kin_config(C.Structure):
    _fields_ = [
        ("leg_offset_x", C.c_double),
        ("leg_offset_y", C.c_double),
        ("leg_calf_length", C.c_double),
        ("leg_thigh_length", C.c_double),
        ("leg_thigh_offset", C.c_double),
        ("contact_force_threshold_up", C.c_double),
        ("contact_force_threshold_down", C.c_double),
        ("redundancy", C.c_int32),
        ("pad_", C.c_int32),
    ]


class lk_kin_frontend_state(C.Structure):
    _fields_ = [
        ("contact", C.c_int32 * 4),
        ("last_acc_z", C.c_float),
        ("last_gyr_z", C.c_float),
        ("last_stamp", C.c_double),
    ]


LK_IMU_MSG_FIXED_BYTES = 312   # a ROS1-serialised sensor_msgs/Imu is 312 + frame_id length bytes


class lk_imu_frontend_state(C.Structure):
    _fields_ = [("last_acc_z", C.c_double), ("last_gyr_z", C.c_double), ("last_stamp", C.c_double)]


class lk_pose(C.Structure):
    _fields_ = [
        ("rot", C.c_double * 9),
        ("pos", C.c_double * 3),
        ("vel", C.c_double * 3),
        ("n_effect", C.c_uint64),
        ("n_buckets", C.c_uint32),
        ("n_updates", C.c_uint32),
    ]


def pose_dtype():
    """numpy view of lk_pose (136 B) for vectorised access to pose buffers."""
    import numpy as np

    return np.dtype(lk_pose)


class lk_bucket_pose(C.Structure):
    _fields_ = [
        ("rot", C.c_double * 9),
        ("pos", C.c_double * 3),
        ("vel", C.c_double * 3),
        ("t", C.c_double),
        ("first_point", C.c_uint64),
        ("n_points", C.c_uint32),
        ("n_effect", C.c_uint32),
    ]


def bucket_pose_dtype():
    """numpy view of lk_bucket_pose (144 B): the records of lk_runs_bucket_poses."""
    import numpy as np

    dt = np.dtype(lk_bucket_pose)
    assert dt.itemsize == C.sizeof(lk_bucket_pose) == 144
    return dt


class lk_ate(C.Structure):
    _fields_ = [
        ("rmse", C.c_double),
        ("mean", C.c_double),
        ("max", C.c_double),
        ("rot", C.c_double * 9),
        ("trans", C.c_double * 3),
        ("n_pairs", C.c_uint64),
        ("worst", C.c_uint32),
        ("status", C.c_uint32),
    ]


LK_ATE_ALIGN = 1       # lk_traj_ate_dev / lk_runs_ate_dev flag: remove the best rigid motion estimate -> ground truth first
LK_ATE_NONFINITE = 1   # lk_ate.status: a paired position was not finite


def ate_dtype():
    """numpy view of lk_ate (136 B): the records of lk_traj_ate_dev / lk_runs_ate_dev."""
    import numpy as np

    dt = np.dtype(lk_ate)
    assert dt.itemsize == C.sizeof(lk_ate) == 136
    return dt


class lk_rpe(C.Structure):
    _fields_ = [
        ("trans_rmse", C.c_double),
        ("trans_mean", C.c_double),
        ("trans_max", C.c_double),
        ("rot_rmse", C.c_double),
        ("rot_mean", C.c_double),
        ("rot_max", C.c_double),
        ("n_terms", C.c_uint64),
        ("n_pairs", C.c_uint64),
        ("worst_trans", C.c_uint32),
        ("worst_rot", C.c_uint32),
        ("status", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


LK_RPE_INDEX = 1       # lk_traj_rpe_dev / lk_runs_rpe_dev flag: delta counts estimate samples instead of seconds
LK_RPE_NONFINITE = 1   # lk_rpe.status: a pose of a term was not finite


def rpe_dtype():
    """numpy view of lk_rpe (80 B): the records of lk_traj_rpe_dev / lk_runs_rpe_dev."""
    import numpy as np

    dt = np.dtype(lk_rpe)
    assert dt.itemsize == C.sizeof(lk_rpe) == 80
    return dt


class lk_c2c(C.Structure):
    _fields_ = [
        ("rmse", C.c_double),
        ("mean", C.c_double),
        ("max", C.c_double),
        ("n_query", C.c_uint64),
        ("n_matched", C.c_uint64),
        ("n_within", C.c_uint64 * 4),
        ("worst", C.c_uint32),
        ("status", C.c_uint32),
    ]


LK_C2C_NONFINITE = 1   # lk_c2c.status: a coordinate of either cloud of the pair was not finite
LK_C2C_RANGE = 2       # lk_c2c.status: |p / max_dist| >= 2^30 in either cloud of the pair
LK_C2C_NO_MATCH = 0xFFFFFFFF   # nn_idx of an unmatched query point (its nn_d2 is +inf)


def c2c_dtype():
    """numpy view of lk_c2c (80 B): the records of lk_clouds_c2c_dev / lk_clouds_c2c."""
    import numpy as np

    dt = np.dtype(lk_c2c)
    assert dt.itemsize == C.sizeof(lk_c2c) == 80
    return dt


class lk_align(C.Structure):
    _fields_ = [
        ("rot", C.c_double * 9),
        ("trans", C.c_double * 3),
        ("rmse_first", C.c_double),
        ("step_rot", C.c_double),
        ("step_trans", C.c_double),
        ("n_matched_first", C.c_uint64),
        ("iters", C.c_uint32),
        ("status", C.c_uint32),
    ]


LK_ALIGN_NONFINITE = 1   # lk_align.status: a coordinate of either INPUT cloud of the pair was not finite
LK_ALIGN_RANGE = 2       # lk_align.status: |p / max_dist| >= 2^30 in either input cloud of the pair
LK_ALIGN_FEW = 4         # lk_align.status: a search matched fewer than 3 points; T is the one of that search
LK_ALIGN_CONVERGED = 8   # lk_align.status: the last solve moved by no more than eps_rot and eps_trans
LK_ALIGN_BAD_T0 = 16     # lk_align.status: T0 of the pair held a non-finite entry


def align_dtype():
    """numpy view of lk_align (136 B): the records of lk_clouds_align_dev / lk_clouds_align."""
    import numpy as np

    dt = np.dtype(lk_align)
    assert dt.itemsize == C.sizeof(lk_align) == 136
    return dt


class lk_mme(C.Structure):
    _fields_ = [
        ("mme", C.c_double),
        ("mpv", C.c_double),
        ("h_max", C.c_double),
        ("n_points", C.c_uint64),
        ("n_dense", C.c_uint64),
        ("n_scored", C.c_uint64),
        ("n_pairs", C.c_uint64),
        ("worst", C.c_uint32),
        ("status", C.c_uint32),
    ]


LK_MME_NONFINITE = 1   # lk_mme.status: a coordinate of the cloud was not finite
LK_MME_RANGE = 2       # lk_mme.status: |p / radius| >= 2^30 in the cloud


def mme_dtype():
    """numpy view of lk_mme (64 B): the records of lk_clouds_mme_dev / lk_clouds_mme."""
    import numpy as np

    dt = np.dtype(lk_mme)
    assert dt.itemsize == C.sizeof(lk_mme) == 64
    return dt


class lk_align_plane(C.Structure):
    _fields_ = [
        ("rmse_plane_first", C.c_double),
        ("rmse_plane", C.c_double),
        ("n_used_first", C.c_uint64),
        ("n_used", C.c_uint64),
    ]


LK_ALIGN_DEGENERATE = 32   # lk_align.status (lk_clouds_align_plane_dev): the used points' normals leave a direction unobserved; T is that search's


def align_plane_dtype():
    """numpy view of lk_align_plane (32 B): the optional records of lk_clouds_align_plane_dev / lk_clouds_align_plane."""
    import numpy as np

    dt = np.dtype(lk_align_plane)
    assert dt.itemsize == C.sizeof(lk_align_plane) == 32
    return dt


class lk_normals(C.Structure):
    _fields_ = [
        ("n_points", C.c_uint64),
        ("n_valid", C.c_uint64),
        ("status", C.c_uint32),
        ("pad", C.c_uint32),
    ]


def normals_dtype():
    """numpy view of lk_normals (24 B): the records of lk_clouds_normals_dev / lk_clouds_normals."""
    import numpy as np

    dt = np.dtype(lk_normals)
    assert dt.itemsize == C.sizeof(lk_normals) == 24
    return dt


class lk_sor(C.Structure):
    _fields_ = [
        ("mu", C.c_double),
        ("sigma", C.c_double),
        ("thr", C.c_double),
        ("n_points", C.c_uint64),
        ("n_isolated", C.c_uint64),
        ("n_outliers", C.c_uint64),
        ("n_kept", C.c_uint64),
        ("worst", C.c_uint32),
        ("status", C.c_uint32),
    ]


LK_SOR_MAX_K = 32       # lk_clouds_sor_dev: the largest k
LK_SOR_NONFINITE = 1    # lk_sor.status: a coordinate of the cloud was not finite
LK_SOR_RANGE = 2        # lk_sor.status: |p / reach| >= 2^30 in the cloud


def sor_dtype():
    """numpy view of lk_sor (64 B): the records of lk_clouds_sor_dev / lk_clouds_sor."""
    import numpy as np

    dt = np.dtype(lk_sor)
    assert dt.itemsize == C.sizeof(lk_sor) == 64
    return dt


class lk_cluster(C.Structure):
    _fields_ = [
        ("n_points", C.c_uint64),
        ("n_core", C.c_uint64),
        ("n_border", C.c_uint64),
        ("n_noise", C.c_uint64),
        ("n_kept", C.c_uint64),
        ("n_clusters", C.c_uint32),
        ("n_kept_clusters", C.c_uint32),
        ("largest", C.c_uint32),
        ("largest_size", C.c_uint32),
        ("status", C.c_uint32),
        ("pad", C.c_uint32),
    ]


LK_CLUSTER_KEEP_LARGEST = 1   # lk_clouds_cluster_dev flags: keep the largest cluster within the size bounds only
LK_CLUSTER_NONFINITE = 1      # lk_cluster.status: a coordinate of the cloud was not finite
LK_CLUSTER_RANGE = 2          # lk_cluster.status: |p / reach| >= 2^30 in the cloud
LK_CLUSTER_NOISE = 0xFFFFFFFF   # d_label of a noise point


def cluster_dtype():
    """numpy view of lk_cluster (64 B): the records of lk_clouds_cluster_dev / lk_clouds_cluster."""
    import numpy as np

    dt = np.dtype(lk_cluster)
    assert dt.itemsize == C.sizeof(lk_cluster) == 64
    return dt


class lk_plane(C.Structure):
    _fields_ = [
        ("normal", C.c_double * 3),
        ("d", C.c_double),
        ("centroid", C.c_double * 3),
        ("eig", C.c_double * 3),
        ("rmse", C.c_double),
        ("n_inliers", C.c_uint32),
        ("hyp", C.c_uint32),
    ]


class lk_planes(C.Structure):
    _fields_ = [
        ("n_points", C.c_uint64),
        ("n_on_planes", C.c_uint64),
        ("n_rest", C.c_uint64),
        ("n_kept", C.c_uint64),
        ("n_planes", C.c_uint32),
        ("status", C.c_uint32),
        ("pad", C.c_uint32 * 6),
    ]


LK_PLANES_MAX_HYP = 4096       # lk_clouds_planes_dev: the most hypotheses of a round
LK_PLANES_MAX_PLANES = 16      # and the most planes of a cloud
LK_PLANES_KEEP_PLANES = 1      # lk_clouds_planes_dev flags: the kept set is the points on planes, not the remainder
LK_PLANES_NONFINITE = 1        # lk_planes.status: a coordinate of the cloud was not finite
LK_PLANES_RANGE = 2            # lk_planes.status: a |coordinate| >= 2^30 in the cloud
LK_PLANES_NONE = 0xFFFFFFFF    # d_label of a point on no plane


def planes_dtype():
    """numpy view of lk_planes (64 B): the per-cloud records of lk_clouds_planes_dev / lk_clouds_planes."""
    import numpy as np

    dt = np.dtype(lk_planes)
    assert dt.itemsize == C.sizeof(lk_planes) == 64
    return dt


def plane_dtype():
    """numpy view of lk_plane (96 B): the per-plane records of lk_clouds_planes_dev / lk_clouds_planes, plane r of cloud c at c * max_planes + r."""
    import numpy as np

    dt = np.dtype(lk_plane)
    assert dt.itemsize == C.sizeof(lk_plane) == 96
    return dt


class lk_run_options(C.Structure):
    _fields_ = [("sliding_thresh", C.c_double), ("half_map_size", C.c_int32), ("pad_", C.c_int32)]


class lk_cloud_layout(C.Structure):
    _fields_ = [("point_step", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32), ("off_z", C.c_uint32),
                ("off_time", C.c_uint32), ("lidar_type", C.c_int32)]


class lk_blob_header(C.Structure):
    _fields_ = [
        ("magic", C.c_uint32),
        ("version", C.c_uint32),
        ("n_roots", C.c_uint32),
        ("n_nodes", C.c_uint32),
        ("n_blocks", C.c_uint32),
        ("block_pts", C.c_uint32),
        ("voxel_size", C.c_double),
        ("max_layer", C.c_int32),
        ("max_points_num", C.c_int32),
        ("bytes", C.c_uint64),
    ]


def blob_header_dtype():
    """numpy view of lk_blob_header (48 B)."""
    import numpy as np

    dt = np.dtype(lk_blob_header)
    assert dt.itemsize == C.sizeof(lk_blob_header)
    return dt


# numpy dtypes of the blob records (for parsing exports in tests / tools)
def blob_dtypes():
    import numpy as np

    root = np.dtype([("key", "<i4", 3), ("node", "<i4")])
    plane = np.dtype(
        [
            ("center", "<f8", 3),
            ("normal", "<f8", 3),
            ("d", "<f4"),
            ("radius", "<f4"),
            ("flags", "<u4"),
            ("points_size", "<i4"),
            ("plane_var", "<f8", 21),
            ("min_ev", "<f4"),
            ("mid_ev", "<f4"),
            ("max_ev", "<f4"),
            ("pad", "<u4", 3),
        ]
    )
    node = np.dtype(
        [
            ("child", "<i4", 8),
            ("voxel_center", "<f8", 3),
            ("quater_length", "<f4"),
            ("layer", "<i4"),
            ("npts", "<i4"),
            ("new_points", "<i4"),
            ("state", "<u4"),
            ("block", "<i4"),
            ("key", "<i4", 3),
            ("list_head", "<i4"),
            ("pad", "<u4", 8),
        ]
    )
    pt = np.dtype([("pw", "<f8", 3), ("var", "<f8", 6)])
    block = np.dtype([("pts", pt, LK_BLOCK_PTS)])
    assert plane.itemsize == 256 and node.itemsize == 128 and pt.itemsize == 72
    return root, node, plane, block


def parse_blob(buf):
    """bytes -> dict(header, roots, nodes, planes, blocks) of numpy structured arrays."""
    import numpy as np

    hd = lk_blob_header.from_buffer_copy(bytes(buf[: C.sizeof(lk_blob_header)]))
    assert hd.magic == LK_BLOB_MAGIC, hex(hd.magic)
    root, node, plane, block = blob_dtypes()
    off = C.sizeof(lk_blob_header)
    mv = memoryview(buf)
    out = {"header": hd}
    for name, dt, n in (("roots", root, hd.n_roots), ("nodes", node, hd.n_nodes), ("planes", plane, hd.n_nodes),
                        ("blocks", block, hd.n_blocks)):
        out[name] = np.frombuffer(mv, dtype=dt, count=n, offset=off)
        off += dt.itemsize * n
    assert off == hd.bytes, (off, hd.bytes)
    return out
