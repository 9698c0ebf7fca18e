/*
 * legkilo_hip.h — C-ABI of liblegkilo_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of Leg-KILO: the per-time-bucket LiDAR ESKF
 * update, i.e. KILO::predictUpdatePoint (legkilo/src/core/slam/KILO.cc:108-233)
 * and what it calls in eskf.cc / voxel_map.cc, plus the bucket loop around it
 * (KILO.cc:367-396).  The reference has no FFI of its own; the boundary is the
 * C++ class surface KILO consumes (eskf.h:46-109, voxel_map.h:180-244).  The
 * C++ mirror of that surface lives in leg-kilo_amd/host/ and calls only the
 * functions declared here.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - every function returns 0 on success or a negative lk_status; nothing
 *     throws across the ABI; lk_last_error() gives the text of the last error.
 *   - plain pointers and sizes only.  Arrays are caller-owned.  Matrices are
 *     ROW-MAJOR fp64 unless a comment says otherwise.  Points are f32.
 *   - a handle = one device + one HIP stream + one voxel map + n_slots filter
 *     slots (slot 0 is "the" filter of the reference; slots >0 exist for batch
 *     replay).  A handle is NOT thread-safe (the reference path is single
 *     threaded: leg_kilo_node.cc:35-38).
 *   - calls are synchronous on return unless the name ends in _async.
 *   - pointers named d_* are DEVICE pointers (HBM-resident); all others host.
 *
 * State vector layout (eskf.h:15-32), LK_STATE_DOUBLES = 36:
 *   x[0..8]  rot_ (3x3 row-major)   x[9..11]  pos_     x[12..14] vel_
 *   x[15..17] ba_   x[18..20] bw_   x[21..23] grav_    x[24..26] imu_a_
 *   x[27..29] imu_w_   x[30..32] bv_   x[33..35] contact_
 * Error-state order (30): rot0 pos3 vel6 ba9 bw12 grav15 imu_a18 imu_w21 bv24 contact27.
 */
#ifndef LEGKILO_HIP_H_
#define LEGKILO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LK_DIM_STATE 30
#define LK_STATE_DOUBLES 36
#define LK_ABI_VERSION 1

typedef enum lk_status {
    LK_OK = 0,
    LK_ERR_INVALID = -1,   /* bad argument */
    LK_ERR_HIP = -2,       /* HIP runtime error (text in lk_last_error) */
    LK_ERR_CAPACITY = -3,  /* a device pool (hash / nodes / point blocks / scan) overflowed */
    LK_ERR_NO_DEVICE = -4, /* no gfx950 device visible; there is NO CPU fallback */
    LK_ERR_STATE = -5,     /* call order violated (e.g. update before set_state) */
    LK_ERR_TIMEOUT = -6    /* a bounded device-side wait of the stream path was given up (fault / pre-empted GPU): the filter keeps its
                              pre-scan state, the map may hold a partial insert - restore it and replay the scan.  Not sticky. */
} lk_status;

/* ESKF::Config (eskf.h:49-65) + VoxelMapConfig (voxel_map.h:41-57) + extrinsics
 * (KILO.cc:74-79) + device capacities.  YAML key names are those of
 * legkilo/config/leg_fusion.yaml. */
typedef struct lk_config {
    /* ESKF::Config, declaration order */
    double vel_process_cov;
    double imu_acc_process_cov;
    double imu_gyr_process_cov;
    double contact_process_cov;
    double acc_bias_process_cov;
    double gyr_bias_process_cov;
    double kin_bias_process_cov;
    double imu_acc_meas_noise;
    double imu_acc_z_meas_noise;
    double imu_gyr_meas_noise;
    double kin_meas_noise;
    double chd_meas_noise;          /* loaded, never used by the reference */
    double contact_meas_noise;      /* loaded, never used by the reference */
    double lidar_point_meas_ratio;
    /* VoxelMapConfig */
    double max_voxel_size;          /* yaml voxel_size */
    double planner_threshold;       /* yaml min_eigen_value */
    double beam_err;                /* degrees */
    double dept_err;                /* metres */
    double sigma_num;
    int32_t max_layer;
    int32_t max_iterations;         /* unused by the reference (voxel_map.h:44) */
    int32_t layer_init_num[5];
    int32_t max_points_num;
    /* extrinsics: p_imu = ext_R * p_lidar + ext_T (KILO.cc:128) */
    double ext_R[9];
    double ext_T[3];
    double gravity;                 /* KILO.cc:50 */
    /* device side */
    int32_t device_id;              /* HIP device ordinal */
    uint32_t n_slots;               /* filter slots (>=1); >1 only for batch replay */
    /* max_roots and the root table.  The table has T = next_pow2(8 * max_roots) slots (at least 128: max_roots >= 16) and is probed linearly.
     * Up to T / 2 root voxels - 4 * max_roots when max_roots is a power of two - everything works: lk_map_build / lk_map_update / the scan
     * entries create roots, every lookup finds them, lk_map_export writes them and lk_map_import, lk_map_clear_outside, lk_map_slide and
     * lk_overlay_commit rebuild the table from them.  A map made ON THE DEVICE may go on to T roots: creation and lookup still work (a lookup
     * of an absent key in a full table ends after one circle of the table) and lk_map_export still writes it - but lk_map_import and
     * lk_overlay_commit refuse more than T / 2 roots with LK_ERR_CAPACITY and leave the handle's map as it was, so such a map cannot be
     * restored from its own host blob by a handle of the same max_roots.  The (T + 1)-th root voxel is LK_ERR_CAPACITY "device pool overflow
     * (bits 0x1 ...)" from a bounded loop: the voxels that exist are still found, the map may hold a part of the refused insert, and the
     * handle goes on once lk_map_import has put a map in.  Size max_roots for the load, not for the limit: probe chains grow quickly
     * above T / 4. */
    uint32_t max_roots;             /* root voxels the hash must hold (table = next pow2 of 8x) */
    uint32_t max_nodes;             /* octree nodes (roots + children) */
    uint32_t max_point_blocks;      /* per-leaf point blocks of LK_BLOCK_PTS points */
    uint32_t max_scan_points;       /* points of the largest scan / bucket batch */
} lk_config;

/* PointType fields the path reads (pcl_types.h:11; x,y,z @0 and curvature @36 of
 * the 48-byte pcl::PointXYZINormal): body-frame xyz + per-point time offset. */
typedef struct lk_point {
    float x, y, z;
    float curvature;
} lk_point;

/* sensor_msgs::Imu fields predictUpdateImu reads (KILO.cc:235-258) */
typedef struct lk_imu {
    double stamp;
    double acc[3];
    double gyr[3];
} lk_imu;

/* common::KinImuMeas (sensor_types.hpp:19-27); contact as int32 (bool in the reference) */
typedef struct lk_kin_imu {
    double time_stamp;
    double foot_pos[4][3];
    double foot_vel[4][3];
    int32_t contact[4];
    double acc[3];
    double gyr[3];
} lk_kin_imu;

/* result of one scan / one replay unit */
typedef struct lk_pose {
    double rot[9];   /* row-major */
    double pos[3];
    double vel[3];
    uint64_t n_effect;   /* success_pts_size_out (KILO.cc:180) */
    uint32_t n_buckets;
    uint32_t n_updates;  /* buckets whose N>0 */
} lk_pose;

/* one time bucket of a replayed run (lk_batch_replay_runs_cloud_dev, lk_batch_replay_overlay_runs_cloud_dev) */
typedef struct lk_bucket_pose {      /* 144 bytes */
    double   rot[9], pos[3], vel[3]; /* first 15 doubles of the state after the bucket: the posterior if
                                        it updated, else the state predicted to the bucket's time */
    double   t;                      /* the bucket's absolute time, t_begin + curvature (KILO.cc:376) */
    uint64_t first_point;            /* index into d_pts of the bucket's first point */
    uint32_t n_points, n_effect;     /* n_effect = matched points; 0 means no update, intensity 0 */
} lk_bucket_pose;

/* ---- map blob (lk_map_export / lk_map_import; also the RCCL broadcast payload) ----
 * blob = lk_blob_header | roots[n_roots] | nodes[n_nodes] | planes[n_nodes] | blocks[n_blocks]
 * All little-endian PODs below; node ids index nodes[]/planes[]; block ids index blocks[]. */
#define LK_BLOB_MAGIC 0x4C4B4D50u /* 'LKMP' */
#define LK_BLOCK_PTS 52           /* >= max_points_num + 1 (voxel_map.cc:199,232) */

typedef struct lk_blob_header {
    uint32_t magic, version;
    uint32_t n_roots, n_nodes, n_blocks, block_pts;
    double voxel_size;
    int32_t max_layer, max_points_num;
    uint64_t bytes;              /* total blob size */
} lk_blob_header;

typedef struct lk_root_rec {     /* one hash entry: Vec3i key -> root node (voxel_map.h:186) */
    int32_t key[3];
    int32_t node;
} lk_root_rec;

/* VoxelPlane (voxel_map.h:96-119), 256 B, the record the residual kernel streams */
#define LK_PLANE_IS_PLANE 1u
#define LK_PLANE_IS_INIT 2u
typedef struct lk_plane_rec {
    double center[3];
    double normal[3];
    float d;
    float radius;
    uint32_t flags;
    int32_t points_size;
    double plane_var[21];        /* upper triangle of the 6x6, row-major: (0,0)(0,1)..(0,5)(1,1).. */
    float min_eigen_value, mid_eigen_value, max_eigen_value;
    uint32_t pad_[3];
} lk_plane_rec;

/* VoxelOctoTree (voxel_map.h:129-176) minus the plane, 128 B */
#define LK_NODE_INIT_OCTO 1u
#define LK_NODE_UPDATE_ENABLE 2u
#define LK_NODE_OCTO_STATE 4u
#define LK_NODE_PTS_DROPPED 8u   /* >LK_BLOCK_PTS first-frame points: only the count is kept */
typedef struct lk_node_rec {
    int32_t child[8];            /* -1 = nullptr */
    double voxel_center[3];
    float quater_length;
    int32_t layer;
    int32_t npts;                /* temp_points_.size() */
    int32_t new_points;
    uint32_t state;
    int32_t block;               /* point block id, -1 = none */
    int32_t key[3];              /* root key (roots only) */
    int32_t list_head;           /* device scratch, always -1 at rest */
    uint32_t pad_[8];
} lk_node_rec;

typedef struct lk_pt_rec {       /* pointWithVar fields the map keeps: point_w + var (sym) */
    double pw[3];
    double var[6];               /* xx xy xz yy yz zz */
} lk_pt_rec;

typedef struct lk_block_rec {
    lk_pt_rec pts[LK_BLOCK_PTS];
} lk_block_rec;

typedef struct lk_handle lk_handle;

/* ---- lifetime ---- */
int lk_abi_version(void);
int lk_create(const lk_config* cfg, lk_handle** out);                  /* ESKF(const Config&) + VoxelMapManager(VoxelMapConfig&) */
void lk_destroy(lk_handle* h);
const char* lk_last_error(const lk_handle* h);                         /* h may be NULL */

/* ---- ESKF surface (eskf.h:46-109); slot = filter slot, 0 for the reference's single filter ---- */
int lk_set_state(lk_handle* h, uint32_t slot, const double* x36, const double* P900);  /* setState + cov() */
int lk_get_state(lk_handle* h, uint32_t slot, double* x36, double* P900);              /* state(), cov() */
int lk_set_Q(lk_handle* h, const double* Q900);                        /* setQ */
int lk_get_Q(lk_handle* h, double* Q900);                              /* Q() */
int lk_init_process_cov_q(lk_handle* h);                               /* initProcessCovQ, eskf.cc:47-62 */
int lk_set_times(lk_handle* h, uint32_t slot, double last_predict_t, double last_update_t); /* KILO.cc:350-351 */
int lk_get_times(lk_handle* h, uint32_t slot, double* last_predict_t, double* last_update_t);
int lk_set_acc_norm(lk_handle* h, double acc_norm);                    /* KILO.cc:349 */
int lk_get_acc_norm(lk_handle* h, double* acc_norm);                   /* acc_norm_ (KILO.h:60): part of a checkpoint */
int lk_get_fx(lk_handle* h, uint32_t slot, double dt, double* Fx900);   /* getFx, eskf.cc:72-81 */
int lk_get_function_f(lk_handle* h, uint32_t slot, double dt, double* f30); /* getFunctionf, eskf.cc:64-70 */
int lk_predict(lk_handle* h, uint32_t slot, double dt, int prop_state, int prop_cov);   /* predict, eskf.cc:83-89 */
/* updateByPoints(ObsShared&), eskf.cc:91-113; h6 is N x 6 ROW-major */
int lk_update_by_points(lk_handle* h, uint32_t slot, const double* h6, const double* z, const double* R, size_t N);
/* updateByImu / updateByKinImu (eskf.cc:125-145): ki_h is M x 30 row-major */
int lk_update_by_imu(lk_handle* h, uint32_t slot, const double* ki_z6, const double* ki_R6);
int lk_update_by_kin_imu(lk_handle* h, uint32_t slot, const double* ki_h, const double* ki_z, const double* ki_R, size_t M);

/* ---- local map sliding: VoxelMapManager::mapSliding voxel_map.cc:552-569, clearMemOutOfMap voxel_map.cc:571-594
 * (configured at KILO.cc:68-70: sliding_thresh, half_map_size, map_sliding_en - the caller's gate; the reference itself
 * never calls them).  `position` is what the reference keeps in the public member position_last_ (voxel_map.h:199);
 * the handle keeps last_slide_position (initially the origin, voxel_map.h:201).  A slide deletes every root voxel
 * whose key is strictly outside [k - half_map_size, k + half_map_size]^3, k = floor(position / max_voxel_size), and
 * compacts the node / point-block pools so that device memory is bounded by the live map.
 * *slid = the reference's return value; *n_removed = deleted root voxels (either may be NULL). */
int lk_map_slide(lk_handle* h, const double* position /*3*/, double sliding_thresh, int32_t half_map_size, int32_t* slid,
                 uint32_t* n_removed);
int lk_map_clear_outside(lk_handle* h, int32_t x_max, int32_t x_min, int32_t y_max, int32_t y_min, int32_t z_max, int32_t z_min,
                         uint32_t* n_removed);
/* read (set = 0) or write (set != 0) last_slide_position - part of a checkpoint */
int lk_map_slide_position(lk_handle* h, int32_t set, double* last3);

/* ---- VoxelMapManager surface (voxel_map.h:180-244) ---- */
/* BuildVoxelMap(rot, rot_cov, pos_cov) with feats_down_world_/feats_down_body_ = the two clouds
 * (xyz f32, n x 3); rot/rot_cov/pos_cov are taken from slot 0 (KILO.cc:339). */
int lk_map_build(lk_handle* h, const float* xyz_world, const float* xyz_body, size_t n);
/* UpdateVoxelMap(const std::vector<pointWithVar>&): pw n x 3, var n x 9 (row-major 3x3) fp64 */
int lk_map_update(lk_handle* h, const double* pw, const double* var9, size_t n);
/* Residual build of KILO.cc:122-210 with the CURRENT state of slot 0, no predict, no update, no
 * insert (config 2).  Outputs per input point: h6 n x 6 row-major, z, R, valid (0/1). */
int lk_residuals(lk_handle* h, const float* xyz_body, size_t n, double* h6, double* z, double* R, uint8_t* valid);
/* VoxelMapManager::build_single_residual(pv, root voxel at key, layer 0, is_success = false, prob = 0, single_ptpl)
 * (voxel_map.cc:363-427, started the way KILO.cc:149-155 starts it) for n caller-held pointWithVar: keys3 n x 3 voxel keys,
 * pw n x 3 (pv.point_w), var9 n x 9 (pv.var, row-major).  Outputs per point: found (a root voxel exists at the key), success
 * (is_success), prob, and of the winning plane normal n x 3, center n x 3, d, dis_to_plane (signed, float as voxel_map.h:92 stores
 * it) and layer (-1 and zeros when no plane was taken).  The map is not modified. */
int lk_match_points(lk_handle* h, size_t n, const int32_t* keys3, const double* pw, const double* var9, uint8_t* found,
                    uint8_t* success, double* prob, double* normal3, double* center3, double* d, float* dis_to_plane,
                    int32_t* layer);
int lk_map_stats(lk_handle* h, uint32_t* n_roots, uint32_t* n_nodes, uint32_t* n_blocks);
int lk_map_export(lk_handle* h, void* blob, size_t* bytes);            /* blob==NULL: size query */
int lk_map_import(lk_handle* h, const void* blob, size_t bytes);
/* device-resident blob for the RCCL broadcast (no host staging): lk_blob_header (version | 0x100) | the handle's whole root hash table
 * (16-byte entries: key x, y, z, root node id or a negative value for a free entry) | nodes | planes | blocks, the three pools as in
 * lk_map_export's blob.  d_blob == NULL: size query; *bytes is rounded up to a multiple of 256, and the bytes behind the last block
 * record are padding that is not written.  Only a handle with the same max_roots can import it. */
int lk_map_export_dev(lk_handle* h, void* d_blob, size_t* bytes);
int lk_map_import_dev(lk_handle* h, const void* d_blob, size_t bytes);

/* ---- KILO path (KILO.cc) ---- */
/* predictUpdatePoint (KILO.cc:108-233) on slot 0: xyz_body n x 3 f32 (one time bucket),
 * xyz_world_out n x 3 f32 (cloud_down_world), intensity_out n f32 (0 / 255), *n_effect += N. */
int lk_update_points(lk_handle* h, double t, const float* xyz_body, size_t n, float* xyz_world_out,
                     float* intensity_out, size_t* n_effect);
int lk_update_imu(lk_handle* h, const lk_imu* imu);                    /* predictUpdateImu, KILO.cc:235-258 */
int lk_update_kin_imu(lk_handle* h, const lk_kin_imu* kin);            /* predictUpdateKinImu, KILO.cc:260-314 */
/* bucket loop of KILO::process (KILO.cc:367-396) on a time-SORTED scan: buckets are runs of
 * exactly equal curvature; IMU (imu_mode_only) or kin+IMU messages with stamp < bucket time are
 * consumed first.  n_imu>0 and n_kin>0 together is invalid.  world_out may be NULL. */
int lk_process_scan(lk_handle* h, const lk_point* sorted_pts, size_t n, double t_begin, const lk_imu* imus,
                    size_t n_imu, const lk_kin_imu* kins, size_t n_kin, float* xyz_world_out, lk_pose* out);
/* same with the scan already resident in HBM (d_pts: n x lk_point) and bucket bounds given by the
 * caller: bucket b covers [bucket_off[b], bucket_off[b+1]) at time t_begin + bucket_dt[b]. */
int lk_process_scan_dev(lk_handle* h, const lk_point* d_pts, size_t n, double t_begin, const uint32_t* bucket_off,
                        const double* bucket_dt, size_t n_buckets, lk_pose* out);
/* A recorded run LIVE, in one call, from device-resident scans and messages (what lk_decode_scans_dev, lk_decode_imu_dev + lk_imu_split_dev or
 * lk_decode_highstate_dev + lk_kin_split_dev leave in HBM): scan s = d_pts[scan_off[s], scan_off[s+1]), time-sorted, starting at t_begin[s], is
 * processed on slot 0 against the handle's map WITH the map insert, s = 0 .. n_scans-1 in order - lk_process_scan on a host copy of the same
 * points and messages, bit for bit: lk_pose (out[s]), state, covariance, time stamps, world cloud, map.  scan_off / t_begin / n_msg are host
 * tables; scan_off[0] may be non-zero (a run's scan 0 is the first frame, lk_first_frame_dev: pass the front end's tables shifted by one) and
 * nothing in front of it is read; n_scans is not bounded by n_slots.  msg_kind / n_msg / d_msgs as for lk_batch_replay_scans_imu_dev / _kin_dev:
 * n_msg[s] device records per scan, concatenated (0: none).  d_world_out (may be NULL, 16-byte aligned): one 16-byte record per point, index-aligned with d_pts -
 * cloud_down_world of every scan as x, y, z, intensity - so the run's registered cloud stays in HBM.  opt (may be NULL): after every scan,
 * lk_map_slide(pose.pos, sliding_thresh, half_map_size); *n_slides counts the slides.  The bucket tables of all scans are built once on the
 * device and a few words per scan are read back; every scan then takes the kernels lk_process_scan would choose for it (grid-resident,
 * scan-resident, per-bucket launches; lk_stream_resident / lk_stream_grid / lk_stream_pipeline / profiling are honoured), and only a scan on
 * the per-bucket launches has its table rows and messages read back.  Synchronous.
 * Refused before anything on the handle changes, naming the scan: LK_ERR_INVALID for n_scans == 0, an empty scan, msg_kind outside 0..2 or
 * non-zero with n_msg NULL, a scan whose curvature decreases or is not finite (the first such scan); LK_ERR_CAPACITY for a scan above
 * max_scan_points.  An error from scan k's own launches (pool capacity, LK_ERR_TIMEOUT) ends the run: *n_done = k, out[0..k) are valid and the
 * handle is what lk_process_scan leaves after that error in scan k of a loop. */
typedef struct lk_run_options {
    double  sliding_thresh;   /* lk_map_slide's arguments, applied after every scan with that scan's position */
    int32_t half_map_size;    /* 0: never slide */
    int32_t pad_;
} lk_run_options;
int lk_run_scans_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin,
                     int msg_kind, const uint32_t* n_msg, const void* d_msgs, const lk_run_options* opt /* may be NULL */,
                     float* d_world_out /* may be NULL */, lk_pose* out /* n_scans, may be NULL */,
                     size_t* n_done /* may be NULL */, uint32_t* n_slides /* may be NULL */);

/* ---- sensor decode: LidarProcessing::{velodyne,ouster,hesai}Handler, lidar_processing.cc:25-108 ----
 * msg_data = sensor_msgs::PointCloud2::data (n_points x point_step bytes).  Keeps every filter_num-th point that is
 * outside the blind radius (lidar_processing.h:96-98), curvature = round((t - t_first) * 500) / 500 in the arithmetic
 * type of the respective handler, input order preserved.  begin/end = LidarScan::lidar_begin_time_/lidar_end_time_.
 * out / d_out must hold n_points records and the first *n_out are the result.  Behind them, the host entry leaves `out` as it was; the
 * rest of d_out's room is the device entry's to use (undefined afterwards). */
typedef struct lk_cloud_layout {
    uint32_t point_step;
    uint32_t off_x, off_y, off_z;   /* float32 fields */
    uint32_t off_time;              /* Velodyne `time` f32 | Ouster `t` u32 | Hesai `timestamp` f64 */
    int32_t lidar_type;             /* 1 Velodyne, 2 Ouster, 3 Hesai (sensor_types.hpp:34) */
} lk_cloud_layout;
int lk_decode_scan(lk_handle* h, const void* msg_data, size_t n_points, const lk_cloud_layout* layout, double time_scale,
                   int filter_num, float blind, double header_stamp, lk_point* out, size_t* n_out, double* begin_time,
                   double* end_time);
int lk_decode_scan_dev(lk_handle* h, const void* d_msg_data, size_t n_points, const lk_cloud_layout* layout, double time_scale,
                       int filter_num, float blind, double header_stamp, lk_point* d_out, size_t* n_out, double* begin_time,
                       double* end_time);

/* ---- the two steps in front of the path, device-resident ----
 * pcl::VoxelGrid centroid filter as used at KILO.cc:356-360 (leaf = yaml voxel_grid_resolution; centroid of x, y, z
 * AND curvature) followed by the time sort of KILO.cc:369-370 (stable).  Cells are emitted in ascending cell index,
 * points of a cell are summed in input order in float32 (PCL leaves both undefined; oracle/preprocess_oracle.py).
 * out_sorted must hold n_raw points; *n_out receives the number of cells. */
int lk_preprocess_scan(lk_handle* h, const lk_point* raw, size_t n_raw, float leaf, lk_point* out_sorted, size_t* n_out);
int lk_preprocess_scan_dev(lk_handle* h, const lk_point* d_raw, size_t n_raw, float leaf, lk_point* d_out_sorted, size_t* n_out);
/* The lidar front end of a recorded run: n_msgs sensor_msgs/PointCloud2 payloads -> per message what lk_decode_scan_dev followed by
 * lk_preprocess_scan_dev give (lidarCallBack + LidarProcessing::processing, lidar_processing.cc:25-108; pcl::VoxelGrid + time sort,
 * KILO.cc:356-370), bit for bit, in one call.  Message s = n_points[s] points of layout->point_step bytes at d_msgs + msg_off[s]
 * (any alignment, gaps allowed); one layout / time_scale / filter_num / blind / leaf for the run.  Outputs: scan s = d_out[scan_off[s],
 * scan_off[s+1]) (d_out: room for sum(n_points) points; scan_off: n_msgs + 1 host entries, first 0), t_begin[s] / t_end[s] =
 * LidarScan::lidar_begin_time_ / lidar_end_time_ (host, may be NULL) - ready for lk_batch_replay_scans(_kin)_dev and lk_kin_split_dev.
 * The tables msg_off / n_points / header_stamp are host arrays of n_msgs entries.  LK_ERR_INVALID, naming the first offending message,
 * for what the two per-scan entries refuse, a message without points, more than 0x7fffffff points in all (split the run), header stamps
 * that decrease (lidarCallBack's time check, ros_interface.cc; the reference clears its cache there), a message that decodes to no
 * points, and a voxel-index overflow in any message; the output is then undefined and the handle stays usable.  Synchronous. */
int lk_decode_scans_dev(lk_handle* h, const void* d_msgs, size_t n_msgs, const uint64_t* msg_off, const uint32_t* n_points,
                        const double* header_stamp, const lk_cloud_layout* layout, double time_scale, int filter_num, float blind,
                        float leaf, lk_point* d_out, uint64_t* scan_off, double* t_begin, double* t_end);
/* raw scan -> pose without the cloud leaving HBM: lk_preprocess_scan_dev + the bucket loop of lk_process_scan
 * (only the n_out x 16 B sorted cloud is read back, for the bucket bounds and the IMU interleave). */
int lk_process_raw_scan(lk_handle* h, const lk_point* raw, size_t n_raw, float leaf, double t_begin, const lk_imu* imus,
                        size_t n_imu, const lk_kin_imu* kins, size_t n_kin, size_t* n_down, lk_pose* out);

/* ---- batch replay (config 5): scans are independent units against the handle's FROZEN map ----
 * scan s uses filter slot s (n_scans <= n_slots); all scans have n_pts points laid out
 * d_pts[s * n_pts + i]; bucket bounds are shared by all scans.  Inserts are disabled. */
int lk_batch_set_priors(lk_handle* h, const double* x36, const double* P900, size_t n_scans); /* per-scan priors */
/* same, priors already resident in HBM (d_x36: n_scans x 36, d_P900: n_scans x 900); asynchronous on the handle's
 * stream - a replay loop re-arms its batch without touching the host */
int lk_batch_set_priors_dev(lk_handle* h, const double* d_x36, const double* d_P900, size_t n_scans);
/* Puts every time bucket of every scan of a device-resident batch (layout of lk_batch_replay_dev) into root-voxel order under the slots' PRIOR
 * poses (lk_batch_set_priors(_dev) first): the 64 points of a residual wave then look at a handful of voxels instead of sixty.  Points keep
 * their bucket; the order inside a bucket is one of the legal outcomes of the reference's sort of equal time stamps (KILO.cc:369), so the
 * replay of d_out is a replay of the same scans.  Once per loaded batch.  d_in and d_out must not overlap; needs 16 B of scratch per point. */
int lk_batch_sort_by_voxel_dev(lk_handle* h, const lk_point* d_in, lk_point* d_out, size_t n_scans, size_t n_pts, const uint32_t* bucket_off,
                               size_t n_buckets);
/* Input order of device-resident batches.  The order of the points INSIDE a time bucket is left open by the reference (KILO.cc:369 sorts by time with an
 * unstable sort; a bucket is a run of equal time stamps), but it decides how fast the batch residual kernel runs: in root-voxel order a wave's 64
 * points look at a handful of voxels, in a random order at sixty (1.4 x slower).  LK_BATCH_ORDER_AUTO (default): lk_batch_replay_dev and
 * lk_batch_replay_async_dev keep track of the batches they are given - (device pointer, shape, bucket bounds) and a stamp of 4 096 sampled points,
 * taken on the device ahead of every replay, no host round trip.  A batch that has come back UNCHANGED twice is, at its third replay, sorted ONCE into
 * a library-owned copy unless every bucket already is in voxel order under the slots' priors (the work of lk_batch_sort_by_voxel_dev: 5.6 ms and 16 B per
 * point for 1 024 x 100 000 points; that call synchronises), and the later replays of that batch read the copy: the same scans in another legal order,
 * equal to the replay of the buffer as given up to the order of floating-point sums.  The caller's buffer is never written.  A batch replayed once or
 * twice (new scans streamed through a staging buffer) is never sorted.  New content in a sorted batch's buffer is noticed by the same stamp: the stamp
 * the copy was made from is kept in a word of its own, and a replay reads the copy only if ITS stamp equals that word - so that replay, and every other
 * replay of the new content that was enqueued before the host heard of the change (lk_batch_replay_async_dev never waits), reads the buffer as given; the
 * count starts again.  Each of the three streams the asynchronous entry rotates over has its own decision word per batch: replays of one buffer in flight
 * on several streams do not decide for each other.  After an in-place edit too small for the sample, call lk_batch_changed.  The two most recently used
 * batches are kept.  (The count is read by the host without waiting; only at the replay that could be the one to sort does the host wait, once per
 * content, for the replays of that batch still in flight - the sort waits for them anyway.)
 * LK_BATCH_ORDER_AS_GIVEN: every batch is replayed where it lies, no copy, no stamp (also: LEGKILO_BATCH_ORDER=0).
 * The entries WITH insert (lk_batch_replay_overlay*_dev) and the ragged entries always replay as given: with the map insert the order inside a bucket
 * decides which points a voxel holds when it is fitted, and the caller's order is the one its checker knows. */
#define LK_BATCH_ORDER_AS_GIVEN 0
#define LK_BATCH_ORDER_AUTO 1
int lk_batch_order(lk_handle* h, int mode);
int lk_batch_changed(lk_handle* h);
/* For a caller who KNOWS a batch will be replayed many times: examine it and make the voxel-ordered copy now, under the priors of slots [0, n_scans)
 * (lk_batch_set_priors(_dev) first), instead of at its third replay.  Synchronous; once per loaded batch.  In LK_BATCH_ORDER_AS_GIVEN no replay would
 * read the copy: the call then returns LK_OK without examining or copying anything (and nothing is remembered for a later LK_BATCH_ORDER_AUTO). */
int lk_batch_prepare_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, const uint32_t* bucket_off, size_t n_buckets);
/* out3 = { batches examined (replayed unchanged often enough), of those sorted into a copy, sorted batches whose buffer later held other content } since lk_create */
int lk_batch_order_stats(lk_handle* h, uint64_t* out3);
int lk_batch_replay_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, double t_begin,
                        const uint32_t* bucket_off, const double* bucket_dt, size_t n_buckets, lk_pose* out);
/* Config 2 ("voxel kNN + point-to-plane residuals only") for a device-resident batch: the residual build of KILO.cc:122-210 for
 * n_scans x n_pts points in one launch, scan s (layout of lk_batch_replay_dev) under the CURRENT state of filter slot s (lk_batch_set_priors(_dev);
 * no predict, no update, no insert), with the rows MATERIALISED in HBM: d_rows8 [n_scans * n_pts][8] = one 64-byte record per point holding what
 * lk_residuals returns in three arrays - h (1 x 6, KILO.cc:195-197), z (KILO.cc:199), R (KILO.cc:208-209) - and d_valid (0 / 1, the point
 * matched a plane).  Records of unmatched points are zero.  16 B read + 65 B written per point.  d_rows8 must be 16-byte aligned.
 * Asynchronous on the handle's stream (lk_synchronize). */
int lk_batch_residuals_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, double* d_rows8, uint8_t* d_valid);
/* Bulk read-out of the filters a batch replay left in slots [first_slot, first_slot + n): state (n x 36: rot 9, pos, vel, ba, bw,
 * grav, imu_a, imu_w, bv, contact) and covariance (n x 900, row-major) - what ESKF::state() / cov() and getRotCov / getPosCov /
 * getVelCov (blocks (0,0), (3,3), (6,6) of P, eskf.h:46-109) give per filter, for all of them with ONE gather kernel instead of one
 * lk_get_state round trip per slot.  Either pointer may be NULL.  _dev: device pointers, asynchronous on the handle's stream (after
 * everything the batch entries enqueued); the host variant synchronises.  Per scan this is SURVEY 8(e)'s result record: pose, P, and
 * the counters of lk_pose. */
int lk_batch_get_states_dev(lk_handle* h, uint32_t first_slot, size_t n, double* d_x36, double* d_P900);
int lk_batch_get_states(lk_handle* h, uint32_t first_slot, size_t n, double* x36, double* P900);
/* Asynchronous, double-buffered variant: the batch uses filter slots [first_slot, first_slot + n_scans); batches whose
 * slot ranges rotate (first_slot = 0, n_scans, [2 n_scans,] 0, ...) run on up to three streams, so the latency-bound update / predict
 * kernels of one batch overlap the residual launches of the others.  d_x36 / d_P900 (device, n_scans x 36 / 900; both NULL =
 * keep the slots' state) arm the priors on the batch's own stream; the poses are copied into host_out (n_scans records;
 * PINNED host memory for a truly asynchronous copy; may be NULL).  Nothing synchronises: lk_synchronize() completes all
 * enqueued batches.  Buffers must stay valid / untouched until then.  first_slot must be a multiple of n_scans (LK_ERR_INVALID
 * otherwise): the stream a batch runs on is a function of its slot range, so equal-sized ranges never overlap partially; a call
 * with a different n_scans than the batches still in flight first drains them. */
int lk_batch_replay_async_dev(lk_handle* h, const lk_point* d_pts, uint32_t first_slot, size_t n_scans, size_t n_pts, double t_begin,
                              const uint32_t* bucket_off, const double* bucket_dt, size_t n_buckets, const double* d_x36,
                              const double* d_P900, lk_pose* host_out);

/* ---- batch replay WITH the map insert (SURVEY.md 8d, config 5 "scan-local insert overlay") ----
 * What KILO::process does per scan - predict, residual, update AND re-projection + UpdateVoxelMap after every bucket (KILO.cc:108-233,
 * :375-395; voxel_map.cc:336-361), so that buckets 2..n of a scan are matched against the planes their own scan has refitted, cut or
 * created - for n_scans independent scans at once.  Every scan (filter slot s) starts from the handle's map and inserts into its own
 * copy-on-write overlay; the handle's map is not changed, and the overlays are discarded by the next replay.  Same argument meaning
 * as lk_batch_replay_dev (priors from lk_batch_set_priors(_dev); synchronous; out may be NULL).  Per slot the result equals
 * lk_process_scan_dev on a handle that holds a private copy of the map.  LK_ERR_CAPACITY when a scan's overlay outgrows its pools
 * (the message names the slot and the sizes in use); LK_ERR_INVALID when a point's voxel key lies outside +-2^20 (the packed keys of
 * the private root tables); LK_ERR_STATE when the handle's map has no frozen-map grid (key box above 2^24 cells).  A refused replay,
 * here and in the recorded-run form below, leaves the slots at the priors it was called with. */
int lk_batch_replay_overlay_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, double t_begin,
                                const uint32_t* bucket_off, const double* bucket_dt, size_t n_buckets, lk_pose* out);
/* The same for a RECORDED run's scans (config 1 / config 4 shape): every scan its own size, its own time buckets (runs of equal curvature,
 * KILO.cc:375-378), its own start time and - msg_kind 1: lk_imu, 2: lk_kin_imu, 0: none - its own messages, applied between the buckets
 * as the loop at KILO.cc:379-390 does (n_msg[s] records of scan s, concatenated in msgs, time-sorted per scan).  Table arguments as for
 * lk_batch_replay_ragged_dev.  Bucket index after bucket index over all scans: messages + predict, residual against base map + the scan's
 * overlay, update, re-projection + UpdateVoxelMap into the overlay (KILO.cc:108-233) - what KILO::process computes for each scan alone on a
 * private copy of the map.  Any bucket size; synchronous; out may be NULL. */
int lk_batch_replay_overlay_ragged_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const uint32_t* n_buckets,
                                       const uint32_t* bucket_off, const double* bucket_dt, const double* t_begin, const uint32_t* n_msg,
                                       const void* msgs, int msg_kind, lk_pose* out);
/* Whole recorded RUNS with the insert, a run per filter slot: run r = the scans run_off[r] .. run_off[r+1) (run_off: n_runs + 1 scan indices, first 0;
 * n_runs <= n_slots, n_scans = run_off[n_runs] is not bounded by n_slots), scan s = d_pts[scan_off[s] .. scan_off[s+1]) sorted by time, its messages
 * n_msg[s] records of d_msgs (DEVICE memory; msg_kind as above) - the tables lk_decode_scans_dev and lk_kin_split_dev / lk_imu_split_dev leave.  The
 * bucket tables are built on the device.  Per scan this is what lk_batch_replay_overlay_ragged_dev does, one KILO::process after the other: across a
 * scan boundary the slot's state, covariance, time stamps and OVERLAY stay (KILO's members), the messages start at the next scan's first record -
 * what a scan's package held beyond its last bucket is never applied (`measure` is a new package per call, KILO.cc:316-399), and at a scan's first
 * bucket all of its own records below that bucket's time are.  Priors from lk_batch_set_priors(_dev); a slot's time stamps start at the t_begin of
 * its run's first scan.  out[s] (n_scans records, may be NULL): the pose after scan s, n_effect / n_buckets / n_updates of that scan alone.
 * Afterwards lk_batch_get_states(_dev) gives the runs' final states, lk_overlay_export(r) run r's overlay; the handle's map is untouched.
 * Synchronous.  Buckets <= 512 points: run-resident, one wave per run (lk_overlay_resident_rounds as above); else launch by launch - same bits.
 * LK_ERR_INVALID: n_runs 0 or above n_slots, run_off[0] != 0, an empty run or scan, a scan not sorted by time (the message names it), a voxel key
 * outside +-2^20; LK_ERR_CAPACITY: a bucket above max_scan_points, pools set by lk_overlay_reserve that overflow (pools the library sized grow and
 * the call runs again); LK_ERR_STATE: no frozen-map grid.  A refused call leaves the slots at their priors. */
int lk_batch_replay_overlay_runs_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off,
                                     const double* t_begin, int msg_kind, const uint32_t* n_msg, const void* d_msgs, lk_pose* out);
/* The same runs on the FROZEN map - localisation against a finished prior map: arguments as for lk_batch_replay_overlay_runs_dev, run r on slot r, but no
 * insert, no overlay pool, and the handle's map unchanged.  Per scan this is what lk_batch_replay_scans_dev does for one scan (frozen-map grid if there
 * is one, hash table otherwise); across a scan boundary the slot's state, covariance and both time stamps stay, the message cursor jumps to the next
 * scan's first record (what a package held beyond its scan's last bucket is never applied), and at a scan's first bucket all of its own records below
 * that bucket's time are applied, one stamped before the previous scan's last bucket included.  out[s] (n_scans records, may be NULL): the pose after
 * scan s, n_effect / n_buckets / n_updates of that scan alone; afterwards lk_batch_get_states(_dev) gives the runs' final states, and the slots'
 * counters are their last scans'.  Synchronous.
 * flags == 0: priors from lk_batch_set_priors(_dev), a slot's time stamps start at the t_begin of its run's first scan.
 * LK_RUNS_CONTINUE: slot r goes on from the state, covariance and time stamps it HOLDS - on a frozen map the filter record is all a run carries, so a
 * run split at any scan boundary into consecutive calls (the first with flags 0) gives the same bits as one call, and a run's length is unbounded.
 * Nothing marks a slot as "in a run": the caller must not have used slots 0 .. n_runs-1 in between (any other batch or class-surface call on them,
 * lk_batch_set_priors, lk_set_times), or the run continues from whatever that left.
 * Buckets <= 512 points: run-resident, one wave per run; larger buckets without messages: launch by launch, same bits; larger buckets WITH messages
 * are refused, as by the other frozen-map entries.
 * LK_ERR_INVALID: n_runs 0 or above n_slots, run_off[0] != 0, an empty run or scan (the message names it), a scan not sorted by time (the message names
 * it), a bad msg_kind, null arguments, unknown flag bits, messages with a bucket above 512 points; LK_ERR_CAPACITY: a bucket above max_scan_points,
 * 2^32 points or messages or more.  Every check comes before the first write to a slot: a refused call leaves the slots as they were. */
#define LK_RUNS_CONTINUE 1u
int lk_batch_replay_runs_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off, const double* t_begin,
                             int msg_kind, const uint32_t* n_msg, const void* d_msgs, uint32_t flags, lk_pose* out);
/* The two run replays with what KILO::process returns beside the pose: the state after EVERY time bucket and the scans registered into the world
 * frame, every bucket's points under that bucket's own state (KILO.cc:130-133, :219-223 - the placement that removes the motion distortion inside a
 * scan).  Arguments, refusals and messages of lk_batch_replay_runs_dev / lk_batch_replay_overlay_runs_dev, which ARE these entries with both outputs
 * NULL; slots, out[] and overlays are left bit for bit as those leave them.
 * d_world_out (DEVICE, may be NULL, 16-byte aligned): one x y z intensity record per point, index-aligned with d_pts (lk_run_scans_dev's layout) -
 * (float)(R_b (ext_R p + ext_t) + p_b) under the state after the point's bucket, intensity 255.0f where that bucket updated (n_effect > 0), else 0.0f.
 * scan_bucket_off (HOST, n_scans + 1 words, may be NULL): scan s owns the records scan_bucket_off[s] .. scan_bucket_off[s+1) of the bucket table.
 * The bucket table (one lk_bucket_pose per time bucket, in d_pts order) is the library's: with either output given the call records it, and
 * lk_runs_bucket_poses(_dev) copy records first_bucket .. first_bucket + n out of it until the handle's next batch replay of ANY kind.  A call with
 * LK_RUNS_CONTINUE records its own chunk only.  With both outputs NULL nothing is recorded.
 * LK_ERR_INVALID: d_world_out not 16-byte aligned (before the first write to a slot), a record range past the table's count; LK_ERR_STATE from the
 * getters: the handle's last batch replay recorded nothing. */
int lk_batch_replay_runs_cloud_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off,
                                   const double* t_begin, int msg_kind, const uint32_t* n_msg, const void* d_msgs, uint32_t flags, lk_pose* out,
                                   float* d_world_out, uint32_t* scan_bucket_off);
int lk_batch_replay_overlay_runs_cloud_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off,
                                           const double* t_begin, int msg_kind, const uint32_t* n_msg, const void* d_msgs, lk_pose* out,
                                           float* d_world_out, uint32_t* scan_bucket_off);
int lk_runs_bucket_poses_dev(lk_handle* h, uint64_t first_bucket, size_t n, lk_bucket_pose* d_out);
int lk_runs_bucket_poses(lk_handle* h, uint64_t first_bucket, size_t n, lk_bucket_pose* out);
/* Absolute trajectory error of n_traj trajectories against ground truth, in HBM: time association, optional closed-form rigid alignment, RMSE / mean /
 * max of the position errors - leg-kilo_amd/tum.py's associate + ate per trajectory, one small record each for the host.  What a caller of the run
 * replays chooses a slot with, and what a localisation sweep over many priors is ranked by.
 * Layout: d_*_t and d_*_pos are DEVICE pointers (8-byte aligned) to the first sample's stamp and to its three position doubles; sample k lies
 * k * stride BYTES further on, one stride for both pointers of a side (a multiple of 8, >= 8 for the stamps and >= 24 for the positions).  A packed
 * [t x y z] table has stride 32; an lk_bucket_pose table has stride 144 with &rec[0].t and &rec[0].pos[0].
 * est_off, gt_off: HOST tables of n_traj + 1 entries, not decreasing; trajectory r owns the samples off[r] .. off[r+1]) of its side.  A range may be
 * empty, off[0] need not be 0, nothing outside the ranges is read.  A trajectory holds fewer than 2^32 - 1 samples on either side.
 * Association: estimate sample i is paired with the ground-truth sample j(i) of the same trajectory that minimises fabs(t_est[i] - t_gt[j]), the
 * EARLIEST j on equal distance (equal ground-truth stamps are allowed), and the pair counts when that fabs(..) - one double subtraction - is
 * <= max_dt.  Every estimate sample decides alone, so a ground-truth sample may serve several estimate samples.  Whenever consecutive stamps of BOTH
 * trajectories lie more than 2 * max_dt apart, these are exactly the pairs of tum.associate.
 * Error: e_i = |g_i - (R p_i + t)| over the pairs (g ground truth, p estimate).  LK_ATE_ALIGN: R, t minimise sum e_i^2 over proper rotations
 * (det R = +1) - tum.ate(pa = gt, pb = est, align=True); one pair gives e = 0; for collinear or coincident pairs R is not unique and any minimiser is
 * returned (the error figures are unique).  Without the flag R = I, t = 0 and e_i = |g_i - p_i|, exactly.
 * out: HOST, n_traj records, every byte written.  Synchronous; no filter slot, no map and no bucket table is touched, the inputs are not modified.
 * A sum is taken in an order that depends on the trajectory's own samples only: a trajectory's record has the same bits whatever else the call holds.
 * LK_ERR_INVALID before anything is launched: n_traj == 0 (or >= 2^31), null pointers or tables, a misaligned pointer, a bad stride, decreasing
 * offsets, 2^32 - 1 samples or more in one trajectory, max_dt not finite or below 0, unknown flag bits.
 * LK_ERR_INVALID found on the device: a trajectory whose stamps, on either side, decrease or are not finite (the message names the first such
 * trajectory and the side); out is then undefined and the handle stays usable.  A non-finite POSITION is not an error of the call - a diverged filter
 * scores NaN and does not abort a sweep: a trajectory with one in a PAIRED sample gets status LK_ATE_NONFINITE, NaN figures, R = I, t = 0, worst = 0
 * and its n_pairs; the other trajectories are unaffected, and positions of unpaired samples are never read.  n_pairs == 0: NaN figures, status 0. */
typedef struct lk_ate {          /* 136 bytes */
    double   rmse, mean, max;    /* of e_i = |g_i - (R p_i + t)| over the pairs; NaN when n_pairs == 0 or LK_ATE_NONFINITE */
    double   rot[9], trans[3];   /* row-major R and t, estimate -> ground truth; identity and 0 without LK_ATE_ALIGN */
    uint64_t n_pairs;
    uint32_t worst;              /* index, within the trajectory's estimate, of the pair with the largest e_i (first on ties) */
    uint32_t status;             /* 0, or LK_ATE_NONFINITE: a PAIRED position was not finite */
} lk_ate;
#define LK_ATE_ALIGN     1u
#define LK_ATE_NONFINITE 1u
int lk_traj_ate_dev(lk_handle* h, size_t n_traj,
                    const double* d_est_t, const double* d_est_pos, size_t est_stride, const uint64_t* est_off,
                    const double* d_gt_t,  const double* d_gt_pos,  size_t gt_stride,  const uint64_t* gt_off,
                    double max_dt, uint32_t flags, lk_ate* out);
/* The same evaluation with the estimate read where it lies: the bucket table the handle's last _cloud run replay recorded (t and pos of its
 * lk_bucket_pose records, no copy).  Run r is the records run_bucket_off[r] .. run_bucket_off[r+1]) (HOST, n_runs + 1 entries, not decreasing) - with
 * the replay's tables, scan_bucket_off[run_off[r]].  LK_ERR_STATE when the handle's last batch replay recorded nothing (the getters' condition),
 * LK_ERR_INVALID for a range past the table's records; otherwise as lk_traj_ate_dev.  The table, the slots and the overlays are left as they are. */
int lk_runs_ate_dev(lk_handle* h, size_t n_runs, const uint64_t* run_bucket_off,
                    const double* d_gt_t, const double* d_gt_pos, size_t gt_stride, const uint64_t* gt_off,
                    double max_dt, uint32_t flags, lk_ate* out);
/* Relative pose error of n_traj trajectories against ground truth, in HBM: drift per step, in translation AND rotation - the second metric beside the
 * ATE, and the one that reads the rotations.  leg-kilo_amd/tum.py's rpe per trajectory, one small record each for the host.
 * Layout: lk_traj_ate_dev's with a third pointer per side.  d_*_rot points at the first sample's nine row-major doubles, body -> world; one stride
 * serves all three pointers of a side (a multiple of 8, >= 72).  A packed [t x y z r00 .. r22] table has stride 104; an lk_bucket_pose table has
 * stride 144 with &rec[0].t, &rec[0].pos[0], &rec[0].rot[0].  Offsets tables, their rules, out (HOST, n_traj records, every byte written) and
 * synchronous completion as for lk_traj_ate_dev; no filter slot, no map and no bucket table is touched, the inputs are not modified.
 * Partner: estimate sample i has the ground-truth partner j(i) exactly as in lk_traj_ate_dev - the minimiser of fabs(t_est[i] - t_gt[j]), the
 * earliest on equal distance, kept when that one rounded subtraction is <= max_dt.  n_pairs counts the samples that have one.
 * Step: in seconds mode target = t_est[i] + delta (one rounded addition) and k(i) is the first index in (i, n_est) with t_est[k] >= target: the search
 * starts behind i, so with duplicate stamps, or a delta the addition swallows, k is still a later sample - never i itself or an earlier equal stamp.
 * With LK_RPE_INDEX k(i) = i + (uint64)delta.  No such k below n_est: sample i gives no term.  There is NO bound on how far t_est[k] lies behind
 * target: on a gappy estimate a step is longer than asked.
 * Term: sample i gives one when i and k(i) both have partners, a = j(i) and b = j(k).  a == b is allowed: against a ground truth sparser than delta
 * the term scores the estimate's own motion.  With (R, p) the estimate and (Q, g) the ground truth:
 *     dRe = R_i^T R_k,  dpe = R_i^T (p_k - p_i),  dRg = Q_a^T Q_b,  dpg = Q_a^T (g_b - g_a),
 *     e_t = |dpe - dpg|,
 *     E = dRg^T dRe,  s = 0.5 |(E21 - E12, E02 - E20, E10 - E01)|,  c = 0.5 (E00 + E11 + E22 - 1),  e_r = atan2(s, c).
 * The matrices are used as given, without re-orthonormalisation: the figure is this formula on those bits (atan2, not acos: at 1e-9 rad acos gives 0
 * or 1.5e-8).  Both motions are in the first pose's own frame, so one fixed rigid transform of a whole trajectory does not change its figures; an
 * estimate equal to its ground truth scores exactly 0.0 in all six.
 * Figures: RMSE, mean and max of e_t (metres) and of e_r (radians) over the terms; worst_* = the i of the largest term, the first on ties.
 * n_terms == 0: NaN figures, worst_* = 0, status 0.  A sum is taken in an order that depends on the trajectory's own samples only: a trajectory's
 * record has the same bits whatever else the call holds.
 * LK_ERR_INVALID before anything is launched: lk_traj_ate_dev's cases, a null or misaligned rot pointer, a stride below 72 (the message names the
 * side), delta not finite or <= 0, with LK_RPE_INDEX a delta that is no whole number in 1 .. 2^32 - 2, unknown flag bits.
 * LK_ERR_INVALID found on the device: stamps that decrease or are not finite, as for lk_traj_ate_dev.  A non-finite POSE is not an error of the call:
 * a trajectory with a non-finite value in any of the four positions or rotations of a TERM gets status LK_RPE_NONFINITE, NaN figures, worst_* = 0 and
 * its n_pairs / n_terms; the other trajectories are unaffected, and poses of samples that take part in no term are never read. */
typedef struct lk_rpe {              /* 80 bytes */
    double   trans_rmse, trans_mean, trans_max;   /* metres; NaN when n_terms == 0 or LK_RPE_NONFINITE */
    double   rot_rmse,   rot_mean,   rot_max;     /* radians */
    uint64_t n_terms;                /* steps that were scored */
    uint64_t n_pairs;                /* estimate samples that found a ground-truth partner (lk_ate's n_pairs) */
    uint32_t worst_trans, worst_rot; /* index i, within the trajectory's estimate, of the first sample of the worst step (first on ties) */
    uint32_t status;                 /* 0, or LK_RPE_NONFINITE: a pose of a term was not finite */
    uint32_t reserved;               /* written 0 */
} lk_rpe;
#define LK_RPE_INDEX     1u   /* delta counts estimate samples instead of seconds */
#define LK_RPE_NONFINITE 1u
int lk_traj_rpe_dev(lk_handle* h, size_t n_traj,
                    const double* d_est_t, const double* d_est_pos, const double* d_est_rot, size_t est_stride, const uint64_t* est_off,
                    const double* d_gt_t,  const double* d_gt_pos,  const double* d_gt_rot,  size_t gt_stride,  const uint64_t* gt_off,
                    double max_dt, double delta, uint32_t flags, lk_rpe* out);
/* The same with the estimate read where it lies: t, pos and rot of the bucket table of the handle's last _cloud run replay, run r = the records
 * run_bucket_off[r] .. run_bucket_off[r+1]) as for lk_runs_ate_dev.  LK_ERR_STATE when the last batch replay recorded nothing, LK_ERR_INVALID for a
 * range past the table's records; otherwise as lk_traj_rpe_dev.  The table, the slots and the overlays are left as they are. */
int lk_runs_rpe_dev(lk_handle* h, size_t n_runs, const uint64_t* run_bucket_off,
                    const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot, size_t gt_stride, const uint64_t* gt_off,
                    double max_dt, double delta, uint32_t flags, lk_rpe* out);
/* Downsampled map clouds from registered points, many files per call: PcdSaver::downsampleAndSave (common/pcd_saver.hpp:114-121) up to and excluding
 * savePCDFileBinaryCompressed - pcl::VoxelGrid<PointXYZINormal> at `leaf` over each file's buffer of frames.
 * File f = the 16-byte x y z intensity records file_off[f] .. file_off[f+1) of d_world (DEVICE, 16-byte aligned, the layout of d_world_out; consecutive
 * frames of a run are contiguous there, so a file is one range).  file_off: HOST, n_files + 1 entries, not decreasing; file_off[0] may be non-zero and
 * nothing in front of it is read.  d_out (DEVICE, 16-byte aligned, room for file_off[n_files] - file_off[0] records, not overlapping the input): file
 * f's result is the records out_off[f] .. out_off[f+1) of it, out_off[0] == 0 (HOST, n_files + 1 entries); nothing behind out_off[n_files] records is
 * written.  Synchronous; the input is not modified, the filter slots and the map are not touched.
 * Per file (oracle/preprocess_oracle.py::voxel_grid_centroid with intensity in the place of curvature): inv = 1.0f / leaf in float, bounds over the
 * file's own points, ijk = floor(p * inv) - min_b, idx = i0 + i1 div0 + i2 div0 div1; one record per occupied cell in ascending idx, each of x y z
 * intensity the float32 sum of the cell's points in INPUT order (frame after frame, point after point) divided by the float count.  Equal idx in two
 * files are two cells.  (The normal and curvature members of cloud_down_world are zero in the reference and stay zero under a centroid.)
 * Index overflow: when div0 div1 div2 > INT32_MAX pcl::VoxelGrid warns "Leaf size is too small for the input dataset" and hands the input on - that
 * file comes out as its input, record for record in input order, and unfiltered[f] = 1 (HOST, n_files bytes, may be NULL; 0 otherwise).  At 0.1 m that
 * is a cloud from about 129 m of extent per axis on: an ordinary run, not an error, and the other files are unaffected.
 * LK_ERR_INVALID before anything is launched: n_files == 0, leaf not finite or <= 0, null tables or pointers, a misaligned d_world or d_out, input and
 * output overlapping, file_off decreasing, an empty file (the message names it: PcdSaver never writes one), more than 0x7fffffff points in all.
 * LK_ERR_INVALID found on the device: a file with a non-finite coordinate or with |p * inv| >= 2^30 (the message names the first such file); d_out is
 * then undefined and the handle stays usable.
 * lk_downsample_clouds: the same from and to HOST memory (world: the records file_off[0] .. file_off[n_files) are uploaded; out: room as for d_out,
 * out_off[n_files] records are written, what lies behind them is left as it was). */
int lk_downsample_clouds_dev(lk_handle* h, const float* d_world, size_t n_files, const uint64_t* file_off, float leaf, float* d_out, uint64_t* out_off,
                             uint8_t* unfiltered);
int lk_downsample_clouds(lk_handle* h, const float* world, size_t n_files, const uint64_t* file_off, float leaf, float* out, uint64_t* out_off,
                         uint8_t* unfiltered);
/* Cloud-to-cloud nearest-neighbour distance (C2C) of many pairs of clouds in one call: how far the points of a query cloud lie from a reference
 * cloud - accuracy against a survey, completeness with the sides exchanged, slot against slot with both sides the same buffer.  The map metric
 * beside lk_runs_ate_dev / lk_runs_rpe_dev: one small record per pair for the host.  leg-kilo_amd/cloudmetrics.py's c2c is the numpy statement.
 * Layout: both sides are 16-byte x y z w float records (d_world_out's and lk_downsample_clouds_dev's d_out), DEVICE, 16-byte aligned; w is never
 * read.  Cloud c of a side = its records off[c] .. off[c+1]) (q_off / r_off: HOST, n_clouds + 1 entries, not decreasing; ranges may be empty,
 * off[0] need not be 0, nothing outside the ranges is read).  d_query and d_ref may be the same buffer or overlap: both are only read.
 * Pair k scores query cloud pair_q[k] against reference cloud pair_r[k] (HOST, n_pairs entries each); a cloud may serve any number of pairs or none.
 * The search structure of a reference cloud is built once per call.
 * Result, for query point q and reference point r, in float64 from the float32 coordinates and without fused multiply-add:
 *     dx = (double)q.x - (double)r.x (dy, dz likewise),  d2 = (dx*dx + dy*dy) + dz*dz,
 * j(i) = the reference index that minimises (d2, j) lexicographically - the smallest index on equal d2.  Point i is MATCHED when
 * d2_i <= max_dist * max_dist (one rounded product), d_i = sqrt(d2_i).  Every decision - matched, j(i), n_within, worst - is taken on d2.  This
 * is a definition by brute force: the grid the library searches is not part of it (its cell edge is max_dist, doubled until the reference
 * cloud's grid holds fewer than 2^31 cells, so clouds kilometres apart under a small max_dist are an ordinary input).
 * d_nn_idx, d_nn_d2 (DEVICE, both or neither): pair k's query point i has its j(i) and d2_i at entry nn_off[k] + i; an unmatched point has
 * 0xffffffff and +inf.  nn_off: HOST, n_pairs + 1 entries, written by the call, nn_off[0] = 0; required with the two outputs, optional without.
 * Nothing behind nn_off[n_pairs] entries is written.
 * out: HOST, n_pairs records, every byte written.  rmse = sqrt(sum d2_i / n_matched), mean = sum d_i / n_matched, max = the largest d_i, over the
 * matched points; n_within[k] counts the matched points with d2_i <= thr[k] * thr[k] (k < n_thr <= 4, thr: HOST).  A sum is taken in an order that
 * depends on the pair's own two clouds only: a pair's record has the same bits whatever else the call holds.
 * A pair with a non-finite coordinate in either cloud gets LK_C2C_NONFINITE, one with |p / max_dist| >= 2^30 in either cloud LK_C2C_RANGE: NaN
 * figures, zero counts, worst 0, its n_query, and 0xffffffff / +inf in its nn entries; the other pairs are unaffected (a diverged slot scores NaN
 * and does not abort a sweep).  Synchronous; no filter slot, map, overlay or bucket table is touched.
 * LK_ERR_INVALID before anything is launched, the message naming the argument: n_pairs == 0, a null table or pointer but for the optional outputs,
 * one of d_nn_idx / d_nn_d2 without the other or both without nn_off, a misaligned pointer, decreasing offsets, a pair index past its side's cloud
 * count, max_dist not finite or <= 0, n_thr > 4, n_thr > 0 with thr NULL, a thr[k] not finite, < 0 or > max_dist, an nn buffer that overlaps an
 * input or the other nn buffer.  LK_ERR_CAPACITY: 2^31 or more reference records in all, a query cloud of 2^32 - 1 records or more, 2^32 or more
 * query points over all pairs.  A refused call writes nothing.
 * lk_clouds_c2c: the same with query, ref, nn_idx and nn_d2 in HOST memory (4- and 8-byte alignment); the two ranges are uploaded for the call. */
typedef struct lk_c2c {            /* 80 bytes */
    double   rmse, mean, max;      /* of d_i over the MATCHED query points; NaN when n_matched == 0 or status != 0 */
    uint64_t n_query, n_matched;
    uint64_t n_within[4];          /* matched points with d2_i <= thr[k] * thr[k]; entries k >= n_thr written 0 */
    uint32_t worst;                /* index within the query cloud of the largest d2_i, the first on ties; 0 when n_matched == 0 */
    uint32_t status;               /* 0, LK_C2C_NONFINITE, LK_C2C_RANGE (bits) */
} lk_c2c;
#define LK_C2C_NONFINITE 1u
#define LK_C2C_RANGE     2u
int lk_clouds_c2c_dev(lk_handle* h,
                      const float* d_query, size_t n_qclouds, const uint64_t* q_off,
                      const float* d_ref,   size_t n_rclouds, const uint64_t* r_off,
                      size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r,
                      double max_dist, const double* thr, uint32_t n_thr,
                      lk_c2c* out, uint32_t* d_nn_idx, double* d_nn_d2, uint64_t* nn_off);
int lk_clouds_c2c(lk_handle* h,
                  const float* query, size_t n_qclouds, const uint64_t* q_off,
                  const float* ref,   size_t n_rclouds, const uint64_t* r_off,
                  size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r,
                  double max_dist, const double* thr, uint32_t n_thr,
                  lk_c2c* out, uint32_t* nn_idx, double* nn_d2, uint64_t* nn_off);
/* Rigid alignment of many pairs of clouds in one call: fine registration (point-to-point ICP) of a query cloud to a reference cloud from an initial
 * guess within max_dist of the answer - what puts a slot's map, which lies in the frame of its first pose, into a survey's frame so that
 * lk_clouds_c2c_dev means something.  The loop runs on the device with no host round trip between iterations.  leg-kilo_amd/cloudmetrics.py's
 * align / transform are the numpy statements.  Point-to-plane is lk_clouds_align_plane_dev below; scale and global (coarse) registration are not offered.
 * The clouds, offsets, pairs, max_dist, thr / n_thr and the optional nn outputs have exactly the layout and rules of lk_clouds_c2c_dev.
 * T0: HOST, n_pairs x 12 doubles, row-major R then t; NULL means the identity.  max_iter: 0 .. 1000.  eps_rot: radians, eps_trans: metres; both
 * finite and >= 0.  out: HOST, one lk_align per pair, every byte written.  c2c_out: HOST, optional, one lk_c2c per pair.
 * Per pair T = (R, t) maps query to reference, r ~ R q + t, and starts as T0[k].  All arithmetic is float64, without fused multiply-add.
 *   search under T  the moved point is m = ((R[3a] * x + R[3a+1] * y) + R[3a+2] * z) + t[a] per axis a, kept in float64 and never rounded to float32;
 *                   dx = m_x - (double)r.x (dy, dz likewise), d2 = (dx*dx + dy*dy) + dz*dz; j(i) minimises (d2, j), the point is matched when
 *                   d2 <= max_dist * max_dist.  A moved point that is not finite or has |m / max_dist| >= 2^30 is unmatched in that search - not
 *                   an error of the pair.  A definition by brute force: the grid is not part of it.
 *   solve           over the n matched points, from the ORIGINAL query points as doubles: pbar = (sum p_i) / n, rbar = (sum r_j(i)) / n,
 *                   S[3a+b] = sum (p_i - pbar)_a (r_j(i) - rbar)_b, R' = the proper rotation of Horn's closed form for S (the one of
 *                   lk_traj_ate_dev's alignment), t' = rbar - R' pbar.  Nothing is composed, so rounding does not build up over the iterations;
 *                   the centroids are taken first and the centred products second, so rounding is of order 2^-53 extent^2 wherever the clouds lie.
 *   step            step_rot = the angle of E = R' R^T as atan2(s, c), s = 0.5 |(E21 - E12, E02 - E20, E10 - E01)|, c = 0.5 (trace E - 1);
 *                   step_trans = |(R' pbar + t') - (R pbar + t)|.
 *   loop            1. search under T.  2. if iters == max_iter, or the pair has stopped, this search is the final one.  3. otherwise, if n < 3:
 *                   LK_ALIGN_FEW, stop - this search is final and T stays.  4. otherwise solve, T = T', iters += 1.  5. if step_rot <= eps_rot
 *                   and step_trans <= eps_trans: LK_ALIGN_CONVERGED, the next search is final.  A pair takes iters + 1 searches; max_iter == 0
 *                   returns T0 with its figures.  (A solve that repeats the one before it to the bit has both steps exactly 0.)
 *   final search    fills c2c_out[k] - the fields and rules of lk_c2c on the moved points, so c2c_out[k].rmse is the rmse under the returned T - and
 *                   the optional d_nn_idx / d_nn_d2 / nn_off.
 * A pair's sums are taken in an order that depends on the pair's own two clouds, T0[k] and the scalar arguments only: its record has the same bits
 * whatever else the call holds.
 * A pair with LK_ALIGN_NONFINITE or LK_ALIGN_RANGE (of the INPUT clouds, as lk_c2c's bits) or LK_ALIGN_BAD_T0 (a non-finite entry in T0[k]) gets T0[k]
 * copied through, NaN figures, n_matched_first 0, iters 0, every nn entry unmatched; the other pairs are unaffected.  T0's rotation is not checked
 * for orthogonality: the first solve replaces it.  Synchronous; no filter slot, map, overlay or bucket table is touched.
 * LK_ERR_INVALID before anything is launched, the message naming the argument: every refusal of lk_clouds_c2c_dev, max_iter > 1000, an eps that is
 * not finite or is < 0, out NULL.  LK_ERR_CAPACITY as for lk_clouds_c2c_dev.  A refused call writes nothing.
 * lk_clouds_align: the same with query, ref, nn_idx and nn_d2 in HOST memory, like lk_clouds_c2c.
 * lk_clouds_transform_dev writes moved clouds: record off[c] + i of d_in goes to entry off[c] - off[0] + i of d_out, x y z the moved point above
 * under T[c] (HOST, n_clouds x 12 doubles) rounded ONCE to float32, w copied bit for bit - a float32 cloud is what lk_clouds_c2c_dev,
 * lk_clouds_mme_dev and a PCD writer take next.  d_out may be exactly d_in + 4 * off[0] floats (in place); any other overlap, a null or misaligned
 * (16 bytes) pointer, decreasing offsets, n_clouds == 0 and a non-finite T entry are LK_ERR_INVALID; 2^32 records or clouds or more LK_ERR_CAPACITY. */
typedef struct lk_align {          /* 136 bytes */
    double   rot[9], trans[3];     /* T: r ~ R q + t */
    double   rmse_first;           /* rmse of the matched distances of the FIRST search (under T0); NaN when none matched */
    double   step_rot, step_trans; /* of the last solve; NaN when iters == 0 */
    uint64_t n_matched_first;
    uint32_t iters;                /* solves taken */
    uint32_t status;               /* LK_ALIGN_* bits */
} lk_align;
#define LK_ALIGN_NONFINITE 1u
#define LK_ALIGN_RANGE     2u
#define LK_ALIGN_FEW       4u
#define LK_ALIGN_CONVERGED 8u
#define LK_ALIGN_BAD_T0    16u
int lk_clouds_align_dev(lk_handle* h,
                        const float* d_query, size_t n_qclouds, const uint64_t* q_off,
                        const float* d_ref,   size_t n_rclouds, const uint64_t* r_off,
                        size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r,
                        double max_dist, const double* thr, uint32_t n_thr,
                        const double* T0, uint32_t max_iter, double eps_rot, double eps_trans,
                        lk_align* out, lk_c2c* c2c_out, uint32_t* d_nn_idx, double* d_nn_d2, uint64_t* nn_off);
int lk_clouds_align(lk_handle* h,
                    const float* query, size_t n_qclouds, const uint64_t* q_off,
                    const float* ref,   size_t n_rclouds, const uint64_t* r_off,
                    size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r,
                    double max_dist, const double* thr, uint32_t n_thr,
                    const double* T0, uint32_t max_iter, double eps_rot, double eps_trans,
                    lk_align* out, lk_c2c* c2c_out, uint32_t* nn_idx, double* nn_d2, uint64_t* nn_off);
int lk_clouds_transform_dev(lk_handle* h, const float* d_in, size_t n_clouds, const uint64_t* off, const double* T, float* d_out);
/* Point-to-plane alignment of many pairs of clouds in one call: lk_clouds_align_dev with the solve replaced by a 6-dof linearised step against the
 * reference's per-point normals - the remedy for matches that slide along walls and floor.  leg-kilo_amd/cloudmetrics.py's align_plane is the
 * numpy statement.  Arguments, layout, rules and refusals are lk_clouds_align_dev's, plus two:
 * d_ref_normals: DEVICE, 16-byte aligned, one 16-byte record (nx ny nz w) per reference record at the same index as d_ref (record r_off[c] + j is the
 * normal of reference point j of cloud c); w is not read.  A normal is used AS GIVEN, not normalised; a record with a non-finite component marks
 * its point as "has no plane".  Any producer may fill the array; lk_clouds_normals_dev is the library's own.
 * pl_out: HOST, optional, one lk_align_plane per pair.  out is lk_align, unchanged, with one more status bit, LK_ALIGN_DEGENERATE.
 * Per pair T = (R, t) starts as T0[k].  All arithmetic is float64, without fused multiply-add.
 *   search under T  exactly lk_clouds_align_dev's; matching ignores the normals, so rmse_first, n_matched_first, c2c_out and the nn outputs mean
 *                   what they mean there.
 *   used set U      the matched points whose reference normal has three finite components.
 *   pass 1          over U with m_i the moved point: n_u, mbar = (sum m_i) / n_u, pbar = (sum p_i) / n_u of the ORIGINAL points, and sum e_i^2,
 *                   e_i = (nx*dx + ny*dy) + nz*dz, dx = m_x - (double)r.x (dy, dz likewise).
 *   too few         n_u < 6: LK_ALIGN_FEW - this search is final and T stays.
 *   pass 2          c_i = m_i - mbar, the row a_i = (c_i x n, n) of six entries, H += a a^T (21 upper terms), g += a e.  The rows are centred on
 *                   mbar, so rounding is of order 2^-53 extent^2 wherever the clouds lie.
 *   solve           D = diag(H)^(-1/2); a diagonal entry <= 0 is LK_ALIGN_DEGENERATE.  Cholesky of D H D in natural order without pivoting; a pivot
 *                   (the diagonal entry before its square root) <= 2^-20 is LK_ALIGN_DEGENERATE - this search is final and T stays.  Otherwise
 *                   x = -D (D H D)^-1 D g = (omega, v).  A single plane, parallel planes, a corridor without end walls leave directions
 *                   unobserved: the entry reports that and does not drift along them.
 *   update          a rotation about mbar, then v: theta = |omega|, dR = the rotation of the unit quaternion (cos(theta/2), sin(theta/2) omega / theta)
 *                   (the identity for theta == 0), R1 = dR R, R' = the proper rotation nearest R1 (Horn's closed form on R1 transposed, which
 *                   returns a rotation as itself), t' = dR (t - mbar) + (mbar + v).  The re-orthonormalisation keeps R a rotation to rounding
 *                   over any max_iter.
 *   step, loop      step_rot and step_trans of lk_clouds_align_dev from T to T' with pbar, its stop rule and its loop, unchanged.
 *   final search    also gives rmse_plane = sqrt(sum e_i^2 / n_u) and n_used = n_u under the returned T; rmse_plane_first and n_used_first are
 *                   those of the first search.  NaN with nothing to average.
 * A pair's sums are taken in an order that depends on its own clouds, normals, T0[k] and the scalar arguments only.  A pair closed by a status of
 * its inputs or of T0 gets NaN and 0 in its lk_align_plane.
 * LK_ERR_INVALID before anything is launched: every refusal of lk_clouds_align_dev, d_ref_normals NULL or misaligned, or overlapping d_nn_idx or
 * d_nn_d2.  A refused call writes nothing.
 * lk_clouds_align_plane: the same with query, ref, ref_normals, nn_idx and nn_d2 in HOST memory. */
typedef struct lk_align_plane {    /* 32 bytes */
    double   rmse_plane_first;     /* rms plane residual over the used points of the FIRST search; NaN when none */
    double   rmse_plane;           /* the same of the final search, under the returned T */
    uint64_t n_used_first, n_used;
} lk_align_plane;
#define LK_ALIGN_DEGENERATE 32u    /* lk_align.status: the normals of the used points leave a direction unobserved; T is the one of that search */
int lk_clouds_align_plane_dev(lk_handle* h,
                              const float* d_query, size_t n_qclouds, const uint64_t* q_off,
                              const float* d_ref,   size_t n_rclouds, const uint64_t* r_off,
                              size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r,
                              double max_dist, const double* thr, uint32_t n_thr,
                              const double* T0, uint32_t max_iter, double eps_rot, double eps_trans,
                              const float* d_ref_normals, lk_align* out, lk_align_plane* pl_out,
                              lk_c2c* c2c_out, uint32_t* d_nn_idx, double* d_nn_d2, uint64_t* nn_off);
int lk_clouds_align_plane(lk_handle* h,
                          const float* query, size_t n_qclouds, const uint64_t* q_off,
                          const float* ref,   size_t n_rclouds, const uint64_t* r_off,
                          size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r,
                          double max_dist, const double* thr, uint32_t n_thr,
                          const double* T0, uint32_t max_iter, double eps_rot, double eps_trans,
                          const float* ref_normals, lk_align* out, lk_align_plane* pl_out,
                          lk_c2c* c2c_out, uint32_t* nn_idx, double* nn_d2, uint64_t* nn_off);
/* Map scores that need NO reference, of many clouds in one call: mean map entropy (MME) and mean plane variance (MPV) over a map cloud itself -
 * both lower for a crisper map.  What a recorded run without ground truth or survey ranks its slots by; beside lk_clouds_c2c_dev, one small record
 * per cloud for the host.  leg-kilo_amd/cloudmetrics.py's mme is the numpy statement.
 * Layout: a cloud is a range of 16-byte x y z w float records (d_world_out's, lk_downsample_clouds_dev's d_out with its out_off as they are), DEVICE,
 * 16-byte aligned; w is never read.  Cloud c = the records off[c] .. off[c+1]) (off: HOST, n_clouds + 1 entries, not decreasing; empty clouds are
 * allowed, off[0] need not be 0, nothing outside the ranges is read).
 * Definition, for point i of a cloud, `radius` r and min_pts; all arithmetic in float64 from the float32 coordinates, without fused multiply-add:
 *   neighbourhood  N_i = { j in the same cloud : d2(i, j) <= r * r }, d2 exactly lk_clouds_c2c_dev's ((dx*dx + dy*dy) + dz*dz), r * r one rounded
 *                  product.  i itself is a member, so n_i = |N_i| >= 1; duplicates are separate points.  The decision is taken on d2: the grid
 *                  that finds the neighbours (cell edge r, doubled as for C2C) is not part of the definition.
 *   offsets        u_j = (double)p_j - (double)p_i per axis, ABOUT THE QUERY POINT: bounded by r, so the sums below carry rounding of order
 *                  2^-53 r^2 wherever the cloud lies (about the origin they would lose |p|^2 / r^2 of that).  s = sum u_j (3 terms),
 *                  M = sum u_j u_j^T (6 terms) over N_i, in an order of the library's that depends on the cloud's own records (and r) only.
 *   classes        DENSE when n_i >= min_pts, else SPARSE.  Dense: C = (M - s s^T / n_i) / (n_i - 1), tr = C00 + C11 + C22, det = the cofactor
 *                  expansion along the first row.  FLAT when det <= 2^-30 * (tr / 3)^3 (tr == 0, all duplicates, included): below that floor
 *                  det is rounding noise of the float32 storage (a tilted wall at 50 m gives 1e-11 .. 8e-11), whose ln must not be averaged.
 *                  A dense point that is not flat is SCORED.
 *   figures        h_i = 0.5 * (3 * ln(2 pi e) + ln det) for a scored point; lmin_i = max(0, smallest eigenvalue of C) for every dense point,
 *                  flat ones included (closed form, absolute error a few ulp of the largest eigenvalue).
 * out: HOST, n_clouds records, every byte written.  mme = mean h_i over the scored points, mpv = mean lmin_i over the dense points, h_max = the
 * largest h_i, worst = its index in the cloud (the first on ties, 0 when none), n_pairs = sum of n_i over all points.  A figure with nothing to
 * average is NaN.  A cloud's sums are taken in an order that depends on that cloud only: its record has the same bits whatever else the call holds.
 * d_n, d_h, d_lmin (DEVICE, each independently optional): record off[c] + i has its n_i, h_i, lmin_i at entry off[c] - off[0] + i; d_h is NaN where
 * the point is not scored, d_lmin NaN where it is sparse.  Nothing behind off[n_clouds] - off[0] entries is written.
 * A cloud with a non-finite coordinate gets LK_MME_NONFINITE, one with |p / radius| >= 2^30 LK_MME_RANGE: NaN figures, zero counts, its n_points,
 * and n = 0 / NaN in its per-point entries; the other clouds of the call are unaffected.  Synchronous; no filter slot, map, overlay or bucket table
 * is touched.
 * LK_ERR_INVALID before anything is launched, the message naming the argument: n_clouds == 0, a null d_clouds, off or out, a misaligned pointer
 * (16 bytes for the clouds, 4 for d_n, 8 for d_h and d_lmin), decreasing offsets, radius not finite or <= 0, min_pts < 4 (below four points det is
 * 0 by rank), an output that overlaps the input or another output.  LK_ERR_CAPACITY: 2^31 or more records in all (the sort's key count, as in
 * C2C), a cloud of 2^32 - 1 records or more.  A refused call writes nothing.
 * lk_clouds_mme: the same with clouds, n, hh and lmin in HOST memory (4- and 8-byte alignment); the range is uploaded for the call and the
 * per-point arrays are copied back. */
typedef struct lk_mme {            /* 64 bytes */
    double   mme, mpv, h_max;      /* mean h over the scored points, mean lmin over the dense ones, the largest h; NaN with nothing to average */
    uint64_t n_points, n_dense, n_scored, n_pairs;
    uint32_t worst;                /* index within the cloud of the largest h_i, the first on ties; 0 when n_scored == 0 */
    uint32_t status;               /* 0, LK_MME_NONFINITE, LK_MME_RANGE (bits) */
} lk_mme;
#define LK_MME_NONFINITE 1u
#define LK_MME_RANGE     2u
int lk_clouds_mme_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts,
                      lk_mme* out, uint32_t* d_n, double* d_h, double* d_lmin);
int lk_clouds_mme(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts,
                  lk_mme* out, uint32_t* n, double* hh, double* lmin);
/* Per-point normals of many clouds in one call: what lk_clouds_align_plane_dev takes as d_ref_normals.  leg-kilo_amd/cloudmetrics.py's normals is
 * the numpy statement.  Layout, offsets, alignment, status bits (LK_MME_NONFINITE, LK_MME_RANGE) and capacity limits are exactly lk_clouds_mme_dev's.
 * Definition, for point i: N_i, s, M and C = (M - s s^T / n_i) / (n_i - 1) are word for word lk_clouds_mme_dev's, so n_i equals its d_n.
 * l0 <= l1 <= l2: the eigenvalues of C, sorted (closed form, absolute error a few ulp of l2).
 *   planarity  w = (l1 - l0) / l2, and w = 0 when l2 <= 0.
 *   validity   VALID when n_i >= min_pts and w >= min_planarity.
 *   record     d_normals (DEVICE, 16-byte aligned, 16 B per record): record off[c] + i has (nx, ny, nz, w) as float32 at entry off[c] - off[0] + i.
 *              n = the unit eigenvector of l0, rounded once to float32; its sign makes the float64 component of largest magnitude positive, the
 *              first such component on ties.  A point that is not valid gets NaN in nx ny nz; it keeps its w when n_i >= min_pts, a sparse
 *              one gets NaN in w too.
 * out: HOST, n_clouds records, every byte written.  A cloud with a status bit has n_valid 0 and NaN in all four floats of its records.
 * LK_ERR_INVALID before anything is launched: lk_clouds_mme_dev's refusals with min_pts < 3 in the place of < 4, min_planarity not finite or outside
 * [0, 1], a null or misaligned d_normals, d_normals overlapping the input.  LK_ERR_CAPACITY as there.  A refused call writes nothing.
 * lk_clouds_normals: the same with clouds and normals in HOST memory (4-byte alignment). */
typedef struct lk_normals {        /* 24 bytes */
    uint64_t n_points, n_valid;
    uint32_t status;               /* 0, LK_MME_NONFINITE, LK_MME_RANGE (bits) */
    uint32_t pad;                  /* written 0 */
} lk_normals;
int lk_clouds_normals_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts, double min_planarity,
                          lk_normals* out, float* d_normals);
int lk_clouds_normals(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts, double min_planarity,
                      lk_normals* out, float* normals);
/* Outliers removed from many map clouds in one call: PCL's RadiusOutlierRemoval and StatisticalOutlierRemoval in one pass, between the voxel grid
 * and a saved, scored or aligned map.  A point needs k neighbours within `reach`, and a mean distance to its k nearest that does not stand out of
 * its cloud's.  leg-kilo_amd/cloudmetrics.py's sor is the numpy statement.
 * Layout, offsets, alignment, status conditions and capacity limits are exactly lk_clouds_mme_dev's, with `reach` in the place of `radius`; w is
 * never interpreted but is COPIED with its record.
 * Definition, by brute force; all arithmetic in float64 from the float32 coordinates, without fused multiply-add; no grid is part of it:
 *   candidates     of point i: every record j != i of the same cloud with d2(i, j) <= reach * reach, d2 exactly lk_clouds_c2c_dev's, reach * reach
 *                  one rounded product.  Exclusion is BY INDEX: a duplicate of i is a candidate at distance 0.  cnt_i = their number, which is
 *                  lk_clouds_mme_dev's d_n at radius == reach, minus 1.
 *   isolated       cnt_i < k: the radius criterion.  dbar_i = NaN, the point is removed and takes no part in the statistics.
 *   dbar_i         otherwise, with d2_(1) <= ... <= d2_(k) the k smallest candidate values (a multiset: equal d2 give equal roots, so which of
 *                  several tied records is taken does not matter), dbar_i = (sqrt(d2_(1)) + ... + sqrt(d2_(k))) / k, the sum taken in that
 *                  ascending order, one term after the other.
 *   statistics     over the n_s non-isolated points of the cloud: mu = (sum dbar_i) / n_s, sigma = sqrt(sum (dbar_i - mu)^2 / (n_s - 1)) - the
 *                  mean first, the centred squares second - and sigma = 0 when n_s == 1; thr = mu + n_sigma * sigma, and thr = +inf when
 *                  n_sigma is +inf (no product is taken: radius-only filtering).  n_s == 0 gives NaN in all three.  Both sums run in an order of
 *                  the library's that depends on the cloud alone: its record has the same bits whatever else the call holds.
 *   kept           not isolated and dbar_i <= thr (a cloud of nothing but duplicates has dbar = mu = thr = 0 and keeps every point).
 *                  n_outliers counts the non-isolated points that are not kept; worst = the index of the largest dbar_i.
 * out: HOST, n_clouds records, every byte written.
 * Outputs, each optional and independent, except that out_off is required with d_out or d_src_idx:
 *   d_out      (DEVICE, 16-byte aligned, room for off[n_clouds] - off[0] records) the kept records of cloud c in INPUT ORDER, all 16 bytes bit for
 *              bit, as records out_off[c] .. out_off[c+1]) of d_out; out_off: HOST, n_clouds + 1 entries, written by the call, out_off[0] == 0.
 *              Nothing behind out_off[n_clouds] records is written.  d_out / out_off are what lk_clouds_c2c_dev, lk_clouds_mme_dev,
 *              lk_clouds_normals_dev and the align entries take as they are.
 *   d_src_idx  (DEVICE, 4-byte aligned, as many entries) for each output record its index within its input cloud: a caller's normals or any other
 *              side array follow the filter with one gather.
 *   d_keep (1 / 0, bytes), d_cnt (uint32), d_dbar (float64, NaN where isolated): per-point arrays, record off[c] + i at entry off[c] - off[0] + i.
 * A cloud with a non-finite coordinate gets LK_SOR_NONFINITE, one with |p / reach| >= 2^30 LK_SOR_RANGE: NaN figures, zero counts but n_points, an
 * empty output range, keep 0, cnt 0 and dbar NaN in its per-point entries; the other clouds of the call are unaffected.  Synchronous; no filter
 * slot, map, overlay or bucket table is touched.
 * LK_ERR_INVALID before anything is launched, the message naming the argument: n_clouds == 0, a null d_clouds, off or out, decreasing offsets,
 * k == 0 or k > LK_SOR_MAX_K, reach not finite or <= 0, n_sigma NaN, < 0 or -inf, d_out or d_src_idx without out_off, a misaligned pointer (16 bytes
 * for the clouds and d_out, 4 for d_src_idx and d_cnt, 8 for d_dbar), an output that overlaps the input or another output.  LK_ERR_CAPACITY as for
 * lk_clouds_mme_dev.  A refused call writes nothing.
 * lk_clouds_sor: the same with clouds, out_cloud, src_idx, keep, cnt and dbar in HOST memory (4-byte alignment for the clouds); the range is
 * uploaded for the call and the arrays that were asked for are copied back. */
#define LK_SOR_MAX_K 32u
#define LK_SOR_NONFINITE 1u
#define LK_SOR_RANGE     2u
typedef struct lk_sor {            /* 64 bytes */
    double   mu, sigma, thr;       /* over the non-isolated points; NaN with nothing to average or status != 0 */
    uint64_t n_points, n_isolated, n_outliers, n_kept;   /* n_points = n_isolated + n_outliers + n_kept when status == 0 */
    uint32_t worst;                /* index within the cloud of the largest dbar_i, the first on ties; 0 when none */
    uint32_t status;               /* 0, LK_SOR_NONFINITE, LK_SOR_RANGE (bits) */
} lk_sor;
int lk_clouds_sor_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, uint32_t k, double reach, double n_sigma,
                      lk_sor* out, float* d_out, uint64_t* out_off, uint32_t* d_src_idx, uint8_t* d_keep, uint32_t* d_cnt, double* d_dbar);
int lk_clouds_sor(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, uint32_t k, double reach, double n_sigma,
                  lk_sor* out, float* out_cloud, uint64_t* out_off, uint32_t* src_idx, uint8_t* keep, uint32_t* cnt, double* dbar);
/* Many map clouds clustered in one call: DBSCAN (Open3D's cluster_dbscan, scikit-learn's DBSCAN), and with min_pts == 1 PCL's
 * EuclideanClusterExtraction - the connected components within `reach`.  It says which points belong together, which none of the per-point entries
 * above can: a detached clump or a ghost trail is locally as dense as a wall and passes lk_clouds_sor_dev; it goes with a minimum cluster size or
 * with LK_CLUSTER_KEEP_LARGEST.  leg-kilo_amd/cloudmetrics.py's cluster is the numpy statement.
 * Layout, offsets, alignment, status conditions and capacity limits are exactly lk_clouds_mme_dev's, with `reach` in the place of `radius`; w is
 * never interpreted but is COPIED with its record.
 * Definition, by brute force; every decision is taken on d2 - exactly lk_clouds_c2c_dev's, in float64 from the float32 coordinates, without fused
 * multiply-add - against reach * reach, one rounded product; no grid is part of it:
 *   neighbourhood  n_i = the number of records j of the same cloud with d2(i, j) <= reach * reach.  i itself counts, and so do duplicates: n_i is
 *                  lk_clouds_mme_dev's d_n at radius == reach and lk_clouds_sor_dev's d_cnt + 1.
 *   CORE           n_i >= min_pts (scikit-learn's and Open3D's convention: the point counts itself).
 *   clusters       the connected components of the graph on the CORE points of one cloud with an edge where d2 <= reach * reach.  A point that
 *                  is not core never carries a link: two clusters that touch only through a border point stay two.
 *   BORDER         not core, with at least one core point within reach.  It joins the cluster of the core point j that minimises (d2, j)
 *                  lexicographically - the smallest index on equal d2, lk_clouds_c2c_dev's rule.  (Not the usual first-visit rule: this one does
 *                  not depend on any order of traversal.)
 *   NOISE          everything else; its label is 0xffffffff.
 *   numbering      the clusters of a cloud are numbered 0 .. n_clusters - 1 in ascending order of their smallest CORE member's index within the
 *                  cloud; a border point with a smaller index does not change the order.
 *   size           of a cluster: its core plus its border members.
 *   kept           a point of a cluster with min_size <= size <= max_size (0 and 1 mean the same for min_size; max_size 0xffffffff: no bound).
 *                  With LK_CLUSTER_KEEP_LARGEST only the points of the largest cluster within those bounds are kept; among clusters of equal
 *                  size the smallest id is the largest.
 * All of it is whole numbers: a cloud's labels, ids, sizes and record have the same bits whatever else the call holds, and from run to run.
 * out: HOST, n_clouds records, every byte written.  largest / largest_size: the largest cluster of the cloud (whatever the bounds) and its size.
 * Outputs, each optional and independent, except that cl_off is required with d_cl_size or d_cl_first and out_off with d_out or d_src_idx:
 *   d_label (uint32: the cluster's id within its cloud, or 0xffffffff), d_kind (bytes: 0 noise, 1 border, 2 core), d_n (uint32: n_i): DEVICE
 *              per-point arrays, record off[c] + i at entry off[c] - off[0] + i.
 *   d_cl_size, d_cl_first  (DEVICE, uint32, room for off[n_clouds] - off[0] entries) cluster k of cloud c at entry cl_off[c] + k: its size and its
 *              smallest core index within the cloud.  cl_off: HOST, n_clouds + 1 entries, written by the call, cl_off[0] == 0.  Nothing behind
 *              cl_off[n_clouds] entries is written.
 *   d_out, out_off, d_src_idx  exactly lk_clouds_sor_dev's: the kept records of cloud c in INPUT ORDER, all 16 bytes bit for bit, as records
 *              out_off[c] .. out_off[c+1]) of d_out, and for each its index within its input cloud.  They are what lk_clouds_c2c_dev,
 *              lk_clouds_mme_dev, lk_clouds_normals_dev, lk_clouds_sor_dev and the align entries take as they are.
 * A cloud with a non-finite coordinate gets LK_CLUSTER_NONFINITE, one with |p / reach| >= 2^30 LK_CLUSTER_RANGE: zero counts but n_points, label
 * 0xffffffff, kind 0 and n 0 in its per-point entries, no clusters and an empty output range; the other clouds of the call are unaffected.
 * Synchronous; no filter slot, map, overlay or bucket table is touched.
 * LK_ERR_INVALID before anything is launched, the message naming the argument: n_clouds == 0, a null d_clouds, off or out, decreasing offsets,
 * reach not finite or <= 0, min_pts == 0, min_size > max_size, an unknown flag, d_cl_size or d_cl_first without cl_off, d_out or d_src_idx without
 * out_off, a misaligned pointer (16 bytes for the clouds and d_out, 4 for the uint32 arrays), an output that overlaps the input or another
 * output.  LK_ERR_CAPACITY as for lk_clouds_mme_dev.  A refused call writes nothing.
 * lk_clouds_cluster: the same with the clouds and every array in HOST memory (4-byte alignment for the clouds); the range is uploaded for the call
 * and the arrays that were asked for are copied back. */
#define LK_CLUSTER_KEEP_LARGEST 1u
#define LK_CLUSTER_NONFINITE 1u
#define LK_CLUSTER_RANGE     2u
typedef struct lk_cluster {        /* 64 bytes */
    uint64_t n_points, n_core, n_border, n_noise, n_kept;   /* n_points = n_core + n_border + n_noise when status == 0 */
    uint32_t n_clusters, n_kept_clusters;
    uint32_t largest, largest_size;   /* id and size of the largest cluster, the smallest id among equals; 0 and 0 when there is no cluster */
    uint32_t status;               /* 0, LK_CLUSTER_NONFINITE, LK_CLUSTER_RANGE (bits) */
    uint32_t pad;                  /* written 0 */
} lk_cluster;
int lk_clouds_cluster_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double reach, uint32_t min_pts, uint32_t min_size,
                          uint32_t max_size, uint32_t flags, lk_cluster* out, uint32_t* d_label, uint8_t* d_kind, uint32_t* d_n, uint32_t* d_cl_size,
                          uint32_t* d_cl_first, uint64_t* cl_off, float* d_out, uint64_t* out_off, uint32_t* d_src_idx);
int lk_clouds_cluster(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double reach, uint32_t min_pts, uint32_t min_size,
                      uint32_t max_size, uint32_t flags, lk_cluster* out, uint32_t* label, uint8_t* kind, uint32_t* n, uint32_t* cl_size,
                      uint32_t* cl_first, uint64_t* cl_off, float* out_cloud, uint64_t* out_off, uint32_t* src_idx);
/* Dominant planes peeled off many map clouds in one call, by RANSAC: PCL's SACSegmentation with SACMODEL_PLANE (axis null) or
 * SACMODEL_PERPENDICULAR_PLANE (axis given; "the floor" is axis = (0,0,1)), repeated on what is left.  It is the step PCL's recipe puts IN FRONT of
 * EuclideanClusterExtraction - without it everything that stands on the floor is one component of lk_clouds_cluster_dev - and it says which planes
 * a cloud consists of, with how many points and what normal each.  Every entry above decides from a point's neighbourhood; this one fits a global
 * model, and needs no cell index.  leg-kilo_amd/cloudmetrics.py's planes is the numpy statement.
 * Layout, offsets, alignment and capacity limits are exactly lk_clouds_mme_dev's; w is never interpreted but is COPIED with its record.
 * Definition, by brute force; all arithmetic is float64 from the float32 coordinates, one rounding per operation, no fused multiply-add; no decision
 * holds a square root or a division.  A ROUND r works on the REMAINDER of a cloud: the m records not yet on a plane, in input order, numbered
 * 0 .. m-1 by their position in the remainder.
 *   sampler     lk_planes_sample(seed, r, h, m): u_k = splitmix64(seed + (r * LK_PLANES_MAX_HYP + h) * 4 + k), k = 0, 1, 2, where splitmix64(x) is
 *               z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31 (mod 2^64).
 *               i0 = mulhi64(u0, m); i1 = mulhi64(u1, m-1), raised by one if >= i0; i2 = mulhi64(u2, m-2), raised by one if >= min(i0, i1) and
 *               then by one if >= max(i0, i1).  Three distinct positions.  The cloud's index is NOT an input: a cloud's result does not depend on
 *               what else the call holds.
 *   hypothesis  h = 0 .. n_hyp-1: a, b, c = the sampled records; u = b - a, v = c - a; mvec = u x v, each component two products and one
 *               subtraction (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx); q = (mx*mx + my*my) + mz*mz.  SKIPPED (score 0) when q is 0 or not
 *               finite, and with an axis when g*g < ((cos_max_angle*cos_max_angle) * q) * aa, g = (mx*ax + my*ay) + mz*az, aa = (ax*ax + ay*ay)
 *               + az*az: the plane's normal is then further than the angle from the axis, either way round.
 *   score       the number of remainder records p with s*s <= t2q, e = p - a, s = (mx*ex + my*ey) + mz*ez, t2q = (dist*dist) * q.  The three
 *               sample points count (their s is 0 or a rounding of it; they are counted by the same test).
 *   winner      the largest score, the smallest h among equal scores.  If that score is < min_inliers the cloud is finished.  Otherwise the
 *               winner's inliers are plane r: they get label r and leave the remainder, and round r + 1 runs on what is left.  A cloud is also
 *               finished at r == max_planes or when m < max(3, min_inliers).
 *   reported, never fed back into a decision: over the plane's inliers the centroid, then the centred 3 x 3 covariance divided by n (sums in an
 *               order that depends on the cloud alone), its eigen-decomposition (lk_eig3.h): eig[3] ascending, normal = the unit eigenvector of
 *               eig[0], with normal . axis >= 0 when an axis is given and otherwise its component of largest magnitude positive (the first on
 *               ties); d = -normal . centroid; rmse = sqrt(max(eig[0], 0)).  Membership is the winning hypothesis's and nothing else.
 * Labels, counts, hyp and the kept records are whole numbers and bits of the input: the same from run to run and whatever else the call holds.
 * out: HOST, n_clouds records, every byte written.  planes: HOST, n_clouds * max_planes records, plane r of cloud c at entry c * max_planes + r,
 * every byte written, unused entries zero.
 * Outputs, each optional and independent, except that out_off is required with d_out or d_src_idx:
 *   d_label    (DEVICE, uint32) per point, record off[c] + i at entry off[c] - off[0] + i: the plane's number, or 0xffffffff.
 *   d_out, out_off, d_src_idx  exactly lk_clouds_sor_dev's.  The kept set is the REMAINDER - ground and wall removal in front of
 *              lk_clouds_cluster_dev - or with LK_PLANES_KEEP_PLANES the points on planes.
 * A cloud with a non-finite coordinate gets LK_PLANES_NONFINITE, one with a |coordinate| >= 2^30 LK_PLANES_RANGE (below it no intermediate of the
 * score overflows): no planes, zero counts but n_points, labels 0xffffffff and an empty output range; the other clouds of the call are unaffected.
 * Synchronous; no filter slot, map, overlay or bucket table is touched.
 * LK_ERR_INVALID before anything is launched, the message naming the argument: n_clouds == 0, a null d_clouds, off, out or planes, decreasing
 * offsets, dist not finite or <= 0, n_hyp 0 or above LK_PLANES_MAX_HYP, max_planes 0 or above LK_PLANES_MAX_PLANES, min_inliers < 3, an axis that
 * is not finite or is zero, cos_max_angle outside [0, 1] or NaN, an unknown flag, d_out or d_src_idx without out_off, a misaligned pointer (16 bytes
 * for the clouds and d_out, 4 for the uint32 arrays), an output that overlaps the input or another output.  LK_ERR_CAPACITY as for
 * lk_clouds_mme_dev.  A refused call writes nothing.
 * lk_clouds_planes: the same with the clouds and every array in HOST memory (4-byte alignment for the clouds). */
#define LK_PLANES_MAX_HYP 4096u
#define LK_PLANES_MAX_PLANES 16u
#define LK_PLANES_KEEP_PLANES 1u
#define LK_PLANES_NONFINITE 1u
#define LK_PLANES_RANGE     2u
typedef struct lk_plane {          /* 96 bytes */
    double normal[3], d;           /* normal . p + d = 0 */
    double centroid[3];
    double eig[3];                 /* of the covariance / n, ascending */
    double rmse;
    uint32_t n_inliers;
    uint32_t hyp;                  /* the winning hypothesis */
} lk_plane;
typedef struct lk_planes {         /* 64 bytes */
    uint64_t n_points, n_on_planes, n_rest, n_kept;   /* n_points = n_on_planes + n_rest when status == 0 */
    uint32_t n_planes;
    uint32_t status;               /* 0, LK_PLANES_NONFINITE, LK_PLANES_RANGE (bits) */
    uint32_t pad[6];               /* written 0 */
} lk_planes;
int lk_clouds_planes_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double dist, uint32_t n_hyp, uint32_t max_planes,
                         uint32_t min_inliers, const double* axis, double cos_max_angle, uint64_t seed, uint32_t flags, lk_planes* out, lk_plane* planes,
                         uint32_t* d_label, float* d_out, uint64_t* out_off, uint32_t* d_src_idx);
int lk_clouds_planes(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double dist, uint32_t n_hyp, uint32_t max_planes,
                     uint32_t min_inliers, const double* axis, double cos_max_angle, uint64_t seed, uint32_t flags, lk_planes* out, lk_plane* planes,
                     uint32_t* label, float* out_cloud, uint64_t* out_off, uint32_t* src_idx);
/* Per-scan overlay capacities: root voxels a scan's inserts may touch or create, octree nodes and live point blocks of those voxels.
 * 0 (default) = sized by the library: a first guess from the scan size (n_pts / 18 roots), afterwards the previous replay's high-water
 * marks + 25 %, and a scan that outgrows such pools makes them grow and the batch run again (no error).  Capacities set HERE are the
 * caller's word: overflowing them fails the replay with LK_ERR_CAPACITY.  Releases pools of another shape.
 * The private root table of a scan has next_pow2(roots + roots / 4) entries and takes keys until every entry is used (100 roots: 128 entries,
 * the 129th voxel overflows).  Growth is bounded: a replay runs again at most four times, each time with what overflowed doubled - a root
 * table that doubles takes point blocks for 4/5 of its entries and half as many child nodes with it - so library-sized pools reach 16 times
 * their root entries.  A scan that needs more (2 200 voxels behind replays of 10-voxel scans of the same size: 128 entries, 2 048 after four
 * doublings) fails with LK_ERR_CAPACITY "overlay pool overflow" like an explicit reserve, the slots back at their priors and the handle
 * usable; an explicit reserve, or a first replay of representative scans, avoids it. */
int lk_overlay_reserve(lk_handle* h, uint32_t roots_per_scan, uint32_t nodes_per_scan, uint32_t blocks_per_scan);
/* The voxels scan `slot` of the LAST overlay replay holds privately - every root voxel its inserts touched or created, whole octrees -
 * as a map blob (lk_map_export's format; blob == NULL: size query).  Voxels not in it are the handle's, unchanged.
 * An overlay refers to the handle's map as it was at the replay (old points and unchanged planes of a copied voxel stay there): export
 * BEFORE the map is changed.  After lk_process_scan / lk_update_points / lk_map_update / lk_map_build / lk_map_import / lk_map_slide /
 * lk_map_clear_outside the call fails with LK_ERR_STATE. */
int lk_overlay_export(lk_handle* h, uint32_t slot, void* blob, size_t* bytes);
/* Slot `slot`'s overlay of the LAST overlay replay becomes part of the handle's map, without the map leaving HBM: afterwards the handle's map is the
 * map a private handle would hold after KILO::process of that slot's scans on a copy of the base map.  Every root voxel the slot holds privately
 * replaces the base voxel of that key as a whole octree, a private root voxel of a key the base map lacks is added, every other voxel stays bit for
 * bit; records are moved, not recomputed, and get new ids (the ranks of a prefix sum: the same call on the same state gives the same ids).
 * Synchronous.  With lk_batch_get_states(_dev) -> lk_batch_set_priors(_dev) this makes windowed mapping of any length out of the replays with
 * insert: replay a window on all slots, choose a slot (with ground truth: lk_runs_ate_dev), commit it, lk_map_slide if wanted, replay the next window.
 * The call commits ONE slot.  The reference has no answer for a voxel two slots changed; the other slots' overlays are stale afterwards, as after any
 * map change: lk_overlay_export and a second lk_overlay_commit answer LK_ERR_STATE until the next replay with insert, and the frozen-map grid is
 * rebuilt by the next batch replay.
 * flags == 0: no filter slot is touched.  LK_COMMIT_ADOPT_FILTER: the whole filter record of `slot` (state, covariance, both time stamps, counters)
 * is also copied to slot 0, device to device, so that lk_process_scan / lk_run_scans_dev go on live from the committed map.
 * LK_ERR_STATE: no overlay pools, or the map has changed since the replay (lk_overlay_export's conditions); LK_ERR_INVALID: slot was not part of the
 * last replay, unknown flag bits; LK_ERR_CAPACITY: surviving + private records exceed max_nodes / max_point_blocks, or twice the root voxels the
 * root table (lk_map_import's rule) - the message gives the counts.  Every refusal comes before the first write: the map is byte-equal afterwards. */
#define LK_COMMIT_ADOPT_FILTER 1u
int lk_overlay_commit(lk_handle* h, uint32_t slot, uint32_t flags);
/* Largest private root / node / point-block count any scan of the last overlay replay reached (any pointer may be NULL). */
int lk_overlay_stats(lk_handle* h, uint32_t* max_roots, uint32_t* max_nodes, uint32_t* max_blocks);
/* What the overlay pools hold right now: total bytes in HBM and the per-scan capacities (root-table entries = root node records,
 * child nodes, point blocks); all 0 before the first overlay replay / after lk_overlay_reserve released them. */
int lk_overlay_pool_bytes(lk_handle* h, uint64_t* bytes, uint32_t* root_entries, uint32_t* child_nodes, uint32_t* blocks);
/* lk_batch_replay_overlay_ragged_dev runs a batch whose buckets all hold <= 512 points (a recorded scan's 2 ms bins, KILO.cc:375-378)
 * SCAN-RESIDENT: one launch carries every scan through its whole bucket chain incl. the insert; a scan whose bucket needs the
 * insert's fallback code stops behind it, the fallback launch runs, and the scans are launched again.  *rounds = launches of the
 * scan kernel in the handle's last such replay (1 + the largest number of stops of any scan), 0 when that replay ran launch by
 * launch (a bucket over 512 points, or LEGKILO_RAG_RESIDENT=0).  Same results either way, bit for bit. */
int lk_overlay_resident_rounds(lk_handle* h, uint32_t* rounds);

/* Ragged batch: the scans of a recorded run differ in size, in their time buckets (KILO.cc:375-378) and in their start
 * time.  Scan s = d_pts[scan_off[s] .. scan_off[s+1]) (scan_off: n_scans + 1 entries) on filter slot s; n_buckets[s] buckets
 * whose bounds (n_buckets[s] + 1 offsets relative to the scan's first point, first 0, last = points in the scan) and time
 * offsets (n_buckets[s] values, added to t_begin[s]) are the next rows of bucket_off / bucket_dt (rows concatenated in
 * scan order).  Empty buckets are skipped.  Frozen map, priors from lk_batch_set_priors(_dev); synchronous; out may be
 * NULL.  What a bucket loop of KILO::process (KILO.cc:375-395) over each scan would give, for all scans at once. */
int lk_batch_replay_ragged_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off,
                               const uint32_t* n_buckets, const uint32_t* bucket_off, const double* bucket_dt,
                               const double* t_begin, lk_pose* out);

/* The same with the IMU messages of each scan (only_imu_use mode): n_imu[s] messages of scan s, rows concatenated in `imus`,
 * time-sorted per scan; every message stamped before a bucket's time is applied (predictUpdateImu, KILO.cc:235-258) before
 * that bucket, as the loop at KILO.cc:379-383 does.  Requires every bucket to hold <= 512 points (what a recorded scan's
 * 2 ms bins hold); LK_ERR_INVALID otherwise. */
int lk_batch_replay_ragged_imu_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off,
                                   const uint32_t* n_buckets, const uint32_t* bucket_off, const double* bucket_dt,
                                   const double* t_begin, const uint32_t* n_imu, const lk_imu* imus, lk_pose* out);

/* Leg-fusion mode (only_imu_use: false): the same with each scan's kinematic + IMU messages (common::KinImuMeas): every message
 * stamped before a bucket's time is applied (predictUpdateKinImu, KILO.cc:260-314; updateByKinImu, eskf.cc:137-145) before
 * that bucket, as the loop at KILO.cc:384-390 does.  Same <= 512 points-per-bucket requirement. */
int lk_batch_replay_ragged_kin_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off,
                                   const uint32_t* n_buckets, const uint32_t* bucket_off, const double* bucket_dt,
                                   const double* t_begin, const uint32_t* n_kin, const lk_kin_imu* kins, lk_pose* out);

/* Recorded-run replay without host-side bucket tables: scan s = d_pts[scan_off[s] .. scan_off[s+1]) (time-sorted, scan_off: n_scans + 1
 * entries, first 0), start time t_begin[s]; the buckets - runs of exactly equal curvature, KILO.cc:375-378 - are found on the
 * device.  msg_kind 0: no messages; 1: n_msg[s] lk_imu records per scan (only_imu_use, KILO.cc:379-383); 2: lk_kin_imu records
 * (leg fusion, KILO.cc:384-390), concatenated in `msgs`.  Equivalent to lk_batch_replay_ragged(_imu/_kin)_dev on tables built
 * from the same scans.  A scan whose curvature decreases somewhere (the sort of KILO.cc:367-370 was skipped) or is NaN is
 * refused with LK_ERR_INVALID before any filter slot is touched. */
int lk_batch_replay_scans_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin,
                              int msg_kind, const uint32_t* n_msg, const void* msgs, lk_pose* out);

/* ---- leg kinematics front end: unitree_legged_msgs/HighState -> lk_kin_imu on the device ----
 * What the reference runs for every /high_state message before the filter sees it: the redundancy filter of
 * RosInterface::kinematicImuCallBack (ros_interface.cc:221-248), Kinematics::processing (kinematics.cc:5-90: leg order
 * FL FR RL RR -> FR FL RR RL, forward kinematics + Jacobian foot velocity in fp64, the hysteresis ContactDetector of
 * kinematics.h per leg), and the kin branch of syncPackage (ros_interface.cc:303-328) that hands the records to the scans.
 * A message is its ROS1 serialisation (fixed size, no length prefixes), LK_HIGHSTATE_BYTES apart. */
#define LK_HIGHSTATE_BYTES 1095

/* Kinematics::Config (kinematics.h) + the yaml key `redundancy`.  Key names are the yaml's. */
typedef struct lk_kin_config {
    double leg_offset_x;
    double leg_offset_y;
    double leg_calf_length;
    double leg_thigh_length;
    double leg_thigh_offset;
    double contact_force_threshold_up;    /* T_on: a foot off the ground touches down at force > T_on */
    double contact_force_threshold_down;  /* T_off: a foot on the ground lifts off at force < T_off (may exceed T_on: diter.yaml) */
    int32_t redundancy;                   /* != 0: drop a message whose imu acc z AND gyr z equal the previous message's */
    int32_t pad_;
} lk_kin_config;

/* What the front end carries from one message to the next: checkpoint it with lk_kin_get_frontend, resume with lk_kin_set_frontend. */
typedef struct lk_kin_frontend_state {
    int32_t contact[4];      /* ContactDetector::in_contact_ per project leg FR FL RR RL (0 / 1) */
    float last_acc_z;        /* the previous message's imu.accelerometer[2] / gyroscope[2], kept or not (the callback's static) */
    float last_gyr_z;
    double last_stamp;       /* stamp of the last kept message (-inf: none yet) */
} lk_kin_frontend_state;

/* Sets the geometry, thresholds and redundancy flag AND resets the carried state: contacts all 1, last acc z / gyr z 0, last stamp -inf. */
int lk_kin_configure(lk_handle* h, const lk_kin_config* cfg);
int lk_kin_get_frontend(lk_handle* h, lk_kin_frontend_state* st);
int lk_kin_set_frontend(lk_handle* h, const lk_kin_frontend_state* st);
/* n messages (n x LK_HIGHSTATE_BYTES, any alignment) -> the *n_out <= n records of the kept ones, in order.  The carried state advances
 * by exactly these messages, so a stream decoded in chunks gives what one call gives.  LK_ERR_STATE before lk_kin_configure;
 * LK_ERR_INVALID when a kept stamp is older than the kept one before it (in the call or carried): the carried state is then unchanged
 * and the output undefined.  _dev: device input, device output (n records of room), synchronous; the host variant copies both ways. */
int lk_decode_highstate(lk_handle* h, const void* msgs, size_t n, lk_kin_imu* out, size_t* n_out);
int lk_decode_highstate_dev(lk_handle* h, const void* d_msgs, size_t n, lk_kin_imu* d_out, size_t* n_out);
/* The kin branch of syncPackage over time-sorted records (lk_decode_highstate_dev's output) and scans with non-decreasing end times
 * scan_end[n_scans] (host): scan s takes the pending records stamped before scan_end[s], and one more stamped exactly scan_end[s] if it
 * took any.  A scan is packaged when the newest record is >= its end time and a record is pending; packaging stops at the first scan that
 * is not.  Outputs (host): n_msg[s] records of packaged scan s (0 for the others), *n_packaged, *n_consumed = sum of n_msg: the records
 * d_kins[0, n_consumed) are those of the packaged scans, concatenated - ready for lk_batch_replay_scans_kin_dev.  Stateless. */
int lk_kin_split_dev(lk_handle* h, const lk_kin_imu* d_kins, size_t n_kins, const double* scan_end, size_t n_scans, uint32_t* n_msg,
                     size_t* n_packaged, size_t* n_consumed);
/* lk_batch_replay_scans_dev with msg_kind 2 and the records already in HBM (d_kins: the n_msg[s] records of each scan, concatenated). */
int lk_batch_replay_scans_kin_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin,
                                  const uint32_t* n_msg, const lk_kin_imu* d_kins, lk_pose* out);

/* ---- IMU front end (only_imu_use mode): sensor_msgs/Imu -> lk_imu on the device ----
 * What the reference runs for every IMU message before the filter sees it: RosInterface::imuCallBack (ros_interface.cc:194-219: the
 * redundancy filter and the time check) and the IMU branch of syncPackage (ros_interface.cc:277-301) that hands the records to the scans.
 * A message is its ROS1 serialisation; message i = the bytes [msg_off[i], msg_off[i+1]) of the buffer (msg_off: n + 1 host entries,
 * non-decreasing, msg_off[0] may be non-zero).  With L the frame_id length the little-endian fields lie at
 *   0 seq u32 | 4 stamp.sec u32 | 8 stamp.nsec u32 | 12 L u32 | 16 frame_id | 16+L orientation 4 f64 | 48+L its covariance 9 f64 |
 *   120+L angular_velocity 3 f64 | 144+L its covariance 9 f64 | 216+L linear_acceleration 3 f64 | 240+L its covariance 9 f64
 * so a message is LK_IMU_MSG_FIXED_BYTES + L bytes and, L changing from message to message, no field has any alignment.
 * Record: stamp = (double)sec + 1e-9 * (double)nsec (ros::Time::toSec), acc = linear_acceleration, gyr = angular_velocity.
 *   - redundancy != 0: message i is dropped when its linear_acceleration.z == the previous MESSAGE's and its angular_velocity.z == the
 *     previous message's - kept or dropped, that one counts (ros_interface.cc:198-204) - and before the first message the carried values,
 *     which after lk_imu_configure are the zeros of the callback's static.  An fp64 ==: -0.0 matches 0.0, NaN never matches.
 *   - the stamps of the kept messages must not decrease, within the call or against the carried last stamp: LK_ERR_INVALID otherwise
 *     (the reference clears its cache there, ros_interface.cc:209-212; here the call is refused, as for HighState).
 *   - a message is valid only if msg_off[i+1] - msg_off[i] == LK_IMU_MSG_FIXED_BYTES + L (in 64 bits).  A length below
 *     LK_IMU_MSG_FIXED_BYTES (or a decreasing msg_off) is refused on the host; a length that disagrees with L is found on the device before
 *     anything behind byte 16 of that message is read: LK_ERR_INVALID, lk_last_error names the first offending message.  No byte outside
 *     [msg_off[0], msg_off[n]) is ever read, whatever L claims.
 *   - the carried state moves only when the call succeeds, and by exactly the call's messages: a stream decoded in chunks gives what one
 *     call gives.  After a refusal the output is undefined.
 *   - LK_ERR_STATE before lk_imu_configure; n >= 2^31 is refused; n == 0 is LK_OK with *n_out = 0.  out / d_out: room for n records. */
#define LK_IMU_MSG_FIXED_BYTES 312
/* What the front end carries from one message to the next: checkpoint it with lk_imu_get_frontend, resume with lk_imu_set_frontend. */
typedef struct lk_imu_frontend_state {
    double last_acc_z;       /* the previous message's linear_acceleration.z / angular_velocity.z, kept or not (the callback's static) */
    double last_gyr_z;
    double last_stamp;       /* stamp of the last kept message (-inf: none yet) */
} lk_imu_frontend_state;
/* Sets the redundancy flag (yaml key `redundancy`) AND resets the carried state: last acc z / gyr z 0.0, last stamp -inf. */
int lk_imu_configure(lk_handle* h, int redundancy);
int lk_imu_get_frontend(lk_handle* h, lk_imu_frontend_state* st);
int lk_imu_set_frontend(lk_handle* h, const lk_imu_frontend_state* st);
/* _dev: device input (d_msgs = byte 0 of the buffer msg_off counts in, any alignment), device output, synchronous; the host variant
 * copies the bytes [msg_off[0], msg_off[n]) and the kept records. */
int lk_decode_imu_dev(lk_handle* h, const void* d_msgs, size_t n, const uint64_t* msg_off, lk_imu* d_out, size_t* n_out);
int lk_decode_imu(lk_handle* h, const void* msgs, size_t n, const uint64_t* msg_off, lk_imu* out, size_t* n_out);
/* The IMU branch of syncPackage (ros_interface.cc:277-301) over time-sorted records (lk_decode_imu_dev's output): the rule, the arguments
 * and the outputs of lk_kin_split_dev word for word, on lk_imu records - ready for lk_batch_replay_scans_imu_dev.  Stateless. */
int lk_imu_split_dev(lk_handle* h, const lk_imu* d_imus, size_t n_imus, const double* scan_end, size_t n_scans, uint32_t* n_msg,
                     size_t* n_packaged, size_t* n_consumed);
/* lk_batch_replay_scans_dev with msg_kind 1 and the records already in HBM (d_imus: the n_msg[s] records of each scan, concatenated). */
int lk_batch_replay_scans_imu_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin,
                                  const uint32_t* n_msg, const lk_imu* d_imus, lk_pose* out);

/* ---- first frame: how KILO::process starts every run (KILO.cc:332-352), on filter slot 0 ----
 * raw / d_raw: the RAW first cloud (lk_decode_scan(_dev)'s output, not voxel-filtered: KILO.cc:336-339 uses cloud_raw), n points;
 * msgs / d_msgs: the first package's n_msg messages - msg_kind 1: lk_imu records (StateInitialByImu, state_initial.hpp:34-72),
 * msg_kind 2: lk_kin_imu records (StateInitialByKinImu, state_initial.hpp:79-117).  In the reference's order:
 *   1. state: the running mean of the messages' acc / gyr in state_initial.hpp's literal order (N starts at 1, the mean starts at the
 *      first message, which the loop visits again; mean += (cur - mean) / N); acc_norm = |mean_acc|, grav = -mean_acc / acc_norm * gravity
 *      (divide, then multiply), bw = mean_gyr, rot = I, every other entry what a fresh ESKF holds (0), P = 1e-6 I, Q as by
 *      lk_init_process_cov_q.  (cov_acc_ / cov_gyr_ are computed by the reference and never read: left out.)
 *   2. cloudLidarToWorld (KILO.cc:89-106) with the state just written: fp64 rot (ext_R p + ext_T) + pos, cast to float.
 *   3. BuildVoxelMap from the two clouds (lk_map_build's work, the clouds staying in HBM).
 *   4. acc_norm (KILO.cc:349; lk_get_acc_norm) and both time stamps = end_time (KILO.cc:350-351; lk_get_times).
 * Refused before anything changes: n == 0 or n_msg == 0 ("Data packet is not ready", KILO.cc:326-329) and msg_kind not 1 or 2 with
 * LK_ERR_INVALID, a non-empty map with LK_ERR_STATE (as lk_map_build), n > max_scan_points with LK_ERR_CAPACITY.  Synchronous. */
int lk_first_frame_dev(lk_handle* h, const lk_point* d_raw, size_t n, double end_time, int msg_kind, const void* d_msgs, size_t n_msg);
int lk_first_frame(lk_handle* h, const lk_point* raw, size_t n, double end_time, int msg_kind, const void* msgs, size_t n_msg);

/* ---- measurement hooks ---- */
int lk_profile_enable(lk_handle* h, int on);                           /* HIP-event timing around each kernel */
int lk_profile_get(lk_handle* h, const char* kernel, uint64_t* launches, double* total_ms);
int lk_profile_reset(lk_handle* h);
int lk_device_malloc(lk_handle* h, void** d_ptr, size_t bytes);
int lk_device_free(lk_handle* h, void* d_ptr);
int lk_memcpy_h2d(lk_handle* h, void* d_dst, const void* src, size_t bytes);
int lk_memcpy_d2h(lk_handle* h, void* dst, const void* d_src, size_t bytes);
int lk_synchronize(lk_handle* h);
/* Pipelined stream path ("insert off the critical chain"): with the pipeline on (on = 1 or LEGKILO_SPEC=1; the
 * default is the sequential order on one stream, which measures faster) the map insert of bucket k (KILO.cc:216-233) runs on a second HIP stream beside
 * the predict + residual pass of bucket k+1, and a verify pass re-evaluates the tiles whose points looked at a root voxel the
 * insert stamped.  Results are those of the sequential order.  lk_stream_stats: out4 = { buckets that went through the
 * HIP-stream pipeline, their residual tiles, tiles its verify pass evaluated again, buckets the scan-resident kernel (below, its own
 * mechanism: LDS flags inside one workgroup) evaluated again after a conflicting insert } since lk_create. */
int lk_stream_pipeline(lk_handle* h, int on);
/* Scan-resident stream kernel: a scan whose time buckets all hold <= 512 points (the reference's own scan shape: 2 ms bins of a dozen
 * points) runs its whole bucket loop - messages, predict, residual, update AND map insert (KILO.cc:375-395, :216-233) - as ONE launch
 * of one resident workgroup instead of several launches per bucket (on by default; on = 0 or LEGKILO_RESIDENT=0: per-bucket
 * launches).  Same device functions, identical results. */
int lk_stream_resident(lk_handle* h, int on);
/* out2 = { scans that went through the scan-resident kernel, launches it needed beyond one per scan } since lk_create.  The generic
 * fallback items of the insert (a voxel that is cut - init_octo_tree / cut_octo_tree, voxel_map.cc:119-183 -, leftovers after a flip to a
 * tree, a root with more than 64 queued points) are not part of the resident kernel: a bucket that produces one ends the launch, the
 * items run as a launch of their own and the resident kernel is launched again from where it stopped (same results; ~30 us per event). */
int lk_stream_resident_stats(lk_handle* h, uint64_t* out2);
/* TEST HOOK (fault injection for the LK_ERR_TIMEOUT path; no product use): bound_ms > 0 - the resident stream kernels' next launches run with
 * this bound on their device-side waits AND one role stops answering at the scan's fourth bucket, so the call fails with LK_ERR_TIMEOUT and
 * must leave the filter at its pre-scan state; 0 - back to normal. */
int lk_test_stall(lk_handle* h, unsigned int bound_ms);
/* Grid-resident stream kernel: a scan whose time buckets all hold > 512 points (and no IMU / kinematic messages between them) runs
 * its whole bucket loop as ONE launch of co-resident workgroups - the phases of the per-bucket launches separated by grid barriers
 * (agent-scope release / acquire hand-offs) instead of kernel boundaries, the rarely needed phases entered only when the device
 * counters ask for them.  Same device functions, identical results.  mode 1 (default): scans whose buckets hold at most 4 096 points
 * (51 two-ms bins of a 100 000-point scan: 2.53 -> 2.34 ms); 2: any size (5 x 20 000: slower than the launches); 0: never.
 * LEGKILO_GRIDSCAN sets the initial mode. */
int lk_stream_grid(lk_handle* h, int mode);
/* Where the last grid-resident launch of up to 32 workgroups ran: one bit per XCC id its working blocks reported (HW_REG_XCC_ID).  Such a
 * launch starts 8 x G blocks of which every eighth works - blocks are observed (not promised) to go to XCD b % 8, so the working ones
 * share one XCD and its L2, and their barriers then need no L2 write-back.  The kernel does not rely on it: the barriers drop the
 * write-back only when this mask, collected on the device behind a full barrier, has exactly one bit. */
int lk_stream_grid_placement(lk_handle* h, uint32_t* xcc_mask);
int lk_stream_stats(lk_handle* h, uint64_t* out4);
void* lk_stream(lk_handle* h);                                         /* the handle's hipStream_t */

#ifdef __cplusplus
}
#endif
#endif /* LEGKILO_HIP_H_ */
