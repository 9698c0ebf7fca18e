// legkilo_hip.hip - the main translation unit of liblegkilo_hip.so (see lk_internal.h)
#define LK_TU_MAIN 1
#include "lk_internal.h"
#include "lk_batch_stamp.h"
#include "lk_cloud_layout.h"

thread_local std::string g_err;

static int create_pools(lk_handle* h, const lk_config* cfg);

extern "C" {

int lk_abi_version(void) { return LK_ABI_VERSION; }

const char* lk_last_error(const lk_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int lk_create(const lk_config* cfg, lk_handle** out) {
    if (!cfg || !out) return fail(nullptr, LK_ERR_INVALID, "lk_create: null argument");
    *out = nullptr;
    if (cfg->max_layer < 0 || cfg->max_layer > LK_MAX_LAYER)
        return fail(nullptr, LK_ERR_INVALID, "max_layer must be in [0,4]");
    if (cfg->max_points_num + 2 > LK_BLOCK_PTS) return fail(nullptr, LK_ERR_INVALID, "max_points_num must be <= 50");
    for (int i = 0; i < 5; ++i)
        if (cfg->layer_init_num[i] + 1 > LK_BLOCK_PTS || cfg->layer_init_num[i] < 1)
            return fail(nullptr, LK_ERR_INVALID, "layer_init_num out of range");
    if (cfg->n_slots < 1 || cfg->max_roots < 16 || cfg->max_nodes < cfg->max_roots || cfg->max_point_blocks < 16 ||
        cfg->max_scan_points < 64)
        return fail(nullptr, LK_ERR_INVALID, "capacities too small");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, LK_ERR_NO_DEVICE, "no HIP device visible (liblegkilo_hip has no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, LK_ERR_INVALID, "device_id out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device_id) != hipSuccess)
        return fail(nullptr, LK_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, LK_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    lk_handle* h = new lk_handle;
    h->cfg = *cfg;
    const int rc = create_pools(h, cfg);
    if (rc != LK_OK) {  // release whatever was allocated before the failure (lk_destroy is null-safe per field)
        const std::string why = h->err;
        lk_destroy(h);
        return fail(nullptr, rc, why);
    }
    *out = h;
    return LK_OK;
}

static int create_pools(lk_handle* h, const lk_config* cfg) {
    HIPCHK(h, hipSetDevice(cfg->device_id));
    HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->side[i], hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
    }
    if (const char* e = getenv("LEGKILO_UPDATE_CLASSIC")) h->wave_update = atoi(e) == 0;
    if (const char* e = getenv("LEGKILO_GRID")) h->grid_enable = atoi(e) != 0;
    if (const char* e = getenv("LEGKILO_BATCH_ORDER")) h->batch_order_mode = atoi(e) != 0;
    HIPCHK(h, pool_alloc(h, &h->d_grid_mm, 8 * sizeof(int)));
    if (const char* e = getenv("LEGKILO_REPLAY_GROUPS")) h->replay_groups = std::min(std::max(atoi(e), 1), (int)lk_handle::kMaxGroups);
    HIPCHK(h, hipEventCreate(&h->ev0));
    HIPCHK(h, hipEventCreate(&h->ev1));
    // parameters
    LkParams& pr = h->pr;
    memcpy(pr.ext_R, cfg->ext_R, sizeof(pr.ext_R));
    memcpy(pr.ext_T, cfg->ext_T, sizeof(pr.ext_T));
    {
        static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        pr.ext_identity = memcmp(cfg->ext_R, I3, sizeof(I3)) == 0 ? 1 : 0;   // +0.0 only: -0.0 entries take the general path
    }
    pr.voxel_size_d = cfg->max_voxel_size;
    pr.voxel_size_f = (float)cfg->max_voxel_size;
    pr.sigma_num = cfg->sigma_num;
    pr.lidar_ratio = cfg->lidar_point_meas_ratio;
    {
        float degree_inc = (float)cfg->beam_err, range_inc = (float)cfg->dept_err;  // float parameters of calcBodyCov
        double sd = std::sin((degree_inc) * 0.017453293);                           // DEG2RAD (pcl_macros.h)
        pr.dir_var = sd * sd;
        pr.range_var = range_inc * range_inc;
    }
    {
        double inv = 1.0 / cfg->max_voxel_size;
        int e = 0;
        bool pow2 = std::frexp(cfg->max_voxel_size, &e) == 0.5;  // mantissa exactly 0.5 <=> power of two
        pr.inv_vs_exact = pow2 ? inv : 0.0;
    }
    pr.planer_threshold = (float)cfg->planner_threshold;
    pr.max_layer = cfg->max_layer;
    pr.max_points_num = cfg->max_points_num;
    for (int i = 0; i < 5; ++i) pr.layer_init_num[i] = cfg->layer_init_num[i];
    // pools
    // load factor <= 1/8: probe chains are what a wave waits for (505 -> 480 us per 20.5 M points against 1/3); 16 B per slot
    h->hash_cap = next_pow2(8u * cfg->max_roots);
    LkMap& m = h->map;
    memset(&m, 0, sizeof(m));
    m.hash_mask = h->hash_cap - 1;
    m.max_nodes = cfg->max_nodes;
    m.max_blocks = cfg->max_point_blocks;
    m.max_scan = cfg->max_scan_points;
    HIPCHK(h, pool_alloc(h, &m.hash, sizeof(int4) * (size_t)h->hash_cap));
    HIPCHK(h, pool_alloc(h, &m.planes, sizeof(lk_plane_rec) * (size_t)m.max_nodes));
    HIPCHK(h, pool_alloc(h, &m.match, sizeof(lk_match_rec) * (size_t)m.max_nodes));
    HIPCHK(h, pool_alloc(h, &m.nodes, sizeof(lk_node_rec) * (size_t)m.max_nodes));
    HIPCHK(h, pool_alloc(h, &m.blocks, sizeof(lk_block_rec) * (size_t)m.max_blocks));
    HIPCHK(h, pool_alloc(h, &m.counters, sizeof(unsigned int) * LK_CTR_COUNT));
    HIPCHK(h, pool_alloc(h, &m.touched, sizeof(int) * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &m.heavy, sizeof(int) * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &m.next, sizeof(int) * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &m.slots, sizeof(int) * (size_t)LK_SLOTS * (size_t)m.max_nodes));
    HIPCHK(h, pool_alloc(h, &m.scratch, sizeof(int) * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &m.groups, sizeof(LkGroup) * 2 * (size_t)m.max_scan));   // leaf-group descriptors, then the fallback items
    HIPCHK(h, pool_alloc(h, &m.gidx, sizeof(int) * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &m.free_list, sizeof(int) * (size_t)m.max_blocks));
    HIPCHK(h, pool_alloc(h, &m.freed_next, sizeof(int) * (size_t)m.max_blocks));
    HIPCHK(h, pool_alloc(h, &m.dirty, sizeof(unsigned int) * (size_t)m.max_nodes));
    HIPCHK(h, hipMemsetAsync(m.dirty, 0, sizeof(unsigned int) * (size_t)m.max_nodes, h->stream));
    HIPCHK(h, pool_alloc(h, &m.newroot, sizeof(unsigned int) * (size_t)(LK_NEWROOT_MASK + 1)));
    HIPCHK(h, hipMemsetAsync(m.newroot, 0, sizeof(unsigned int) * (size_t)(LK_NEWROOT_MASK + 1), h->stream));
    HIPCHK(h, pool_alloc(h, &m.spec, sizeof(unsigned int) * LK_SPEC_WORDS));
    HIPCHK(h, hipMemsetAsync(m.spec, 0, sizeof(unsigned int) * LK_SPEC_WORDS, h->stream));
    m.epoch = 0;
    HIPCHK(h, hipStreamCreateWithFlags(&h->ins, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_U[i], hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_D[i], hipEventDisableTiming));
    }
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_I, hipEventDisableTiming));
    if (const char* e = getenv("LEGKILO_SPEC")) h->spec_enable = atoi(e) != 0;
    if (const char* e = getenv("LEGKILO_RESIDENT")) h->resident_enable = atoi(e) != 0;
    if (const char* e = getenv("LEGKILO_GRIDSCAN")) h->gridscan_mode = std::min(std::max(atoi(e), 0), 2);
    HIPCHK(h, pool_alloc(h, &h->d_snap, sizeof(LkFilter) * 2));
    HIPCHK(h, hipMemsetAsync(h->d_snap, 0, sizeof(LkFilter) * 2, h->stream));
    HIPCHK(h, pool_alloc(h, &h->d_ids, sizeof(int2) * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &h->d_filters, sizeof(LkFilter) * (size_t)cfg->n_slots));
    HIPCHK(h, hipMemsetAsync(h->d_filters, 0, sizeof(LkFilter) * (size_t)cfg->n_slots, h->stream));
    HIPCHK(h, pool_alloc(h, &h->d_Q, sizeof(double) * 900));
    HIPCHK(h, hipMemsetAsync(h->d_Q, 0, sizeof(double) * 900, h->stream));
    size_t nblk_max = ((size_t)m.max_scan + LK_RB - 1) / LK_RB;
    h->part_stride = nblk_max * (LK_RB / LK_WAVE) * LK_NPART;  // one partial record per wave
    HIPCHK(h, pool_alloc(h, &h->d_partials, sizeof(double) * h->part_stride * cfg->n_slots));
    HIPCHK(h, pool_alloc(h, &h->d_scan, sizeof(lk_point) * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &h->d_world, sizeof(float) * 4 * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &h->d_rows, sizeof(double) * 8 * (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &h->d_valid, (size_t)m.max_scan));
    HIPCHK(h, pool_alloc(h, &h->d_tmp, sizeof(double) * 4096));
    HIPCHK(h, pool_alloc(h, &h->d_poses, sizeof(lk_pose) * (size_t)cfg->n_slots));
    unsigned int ninit = std::max(h->hash_cap, m.max_nodes);
    hipLaunchKernelGGL(lk_pool_init_kernel, dim3((ninit + 255) / 256), dim3(256), 0, h->stream, m, h->hash_cap);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

void lk_destroy(lk_handle* h) {
    if (!h) return;
    hipSetDevice(h->cfg.device_id);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->ins) hipStreamSynchronize(h->ins);
    for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i)   // an asynchronous batch may still be running on a side stream
        if (h->side[i]) hipStreamSynchronize(h->side[i]);
    for (DevBuf* b : h->grown) buf_release(*b);
    for (void* p : h->pools) hipFree(p);
    if (h->h_result) hipHostFree(h->h_result);
    ov_free(h);
    for (auto& e : h->ord) {
        if (e.copy) hipFree(e.copy);
        if (e.d_ref) hipFree(e.d_ref);
        if (e.h_seen) hipHostFree(e.h_seen);
    }
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    for (int i = 0; i < 2; ++i) {
        if (h->ev_U[i]) hipEventDestroy(h->ev_U[i]);
        if (h->ev_D[i]) hipEventDestroy(h->ev_D[i]);
    }
    if (h->ev_I) hipEventDestroy(h->ev_I);
    if (h->ins) hipStreamDestroy(h->ins);
    for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i) {
        if (h->ev_join[i]) hipEventDestroy(h->ev_join[i]);
        if (h->side[i]) hipStreamDestroy(h->side[i]);
    }
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}


// ------------------------------------------------------------------ ESKF surface
int lk_set_state(lk_handle* h, uint32_t slot, const double* x36, const double* P900) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    LkFilter* f = h->d_filters + slot;
    if (x36) HIPCHK(h, hipMemcpyAsync(f->x, x36, sizeof(double) * 36, hipMemcpyHostToDevice, h->stream));
    if (P900) HIPCHK(h, hipMemcpyAsync(f->P, P900, sizeof(double) * 900, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_get_state(lk_handle* h, uint32_t slot, double* x36, double* P900) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    LkFilter* f = h->d_filters + slot;
    if (x36) HIPCHK(h, hipMemcpyAsync(x36, f->x, sizeof(double) * 36, hipMemcpyDeviceToHost, h->stream));
    if (P900) HIPCHK(h, hipMemcpyAsync(P900, f->P, sizeof(double) * 900, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_set_Q(lk_handle* h, const double* Q900) {
    CHECK_H(h);
    if (!Q900) return fail(h, LK_ERR_INVALID, "Q is null");
    h->q_diag = true;
    for (int i = 0; i < 30 && h->q_diag; ++i)
        for (int j = 0; j < 30; ++j)
            if (i != j && Q900[i * 30 + j] != 0.0) {
                h->q_diag = false;
                break;
            }
    HIPCHK(h, hipMemcpyAsync(h->d_Q, Q900, sizeof(double) * 900, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_get_Q(lk_handle* h, double* Q900) {
    CHECK_H(h);
    HIPCHK(h, hipMemcpyAsync(Q900, h->d_Q, sizeof(double) * 900, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
// initProcessCovQ, eskf.cc:47-62 (diagonal blocks only; built on the host, it is 7 scalars)
static int init_process_cov_q(lk_handle* h) {
    std::vector<double> Q(900, 0.0);
    auto diag3 = [&](int o, double v) {
        for (int k = 0; k < 3; ++k) Q[(o + k) * 30 + (o + k)] = v;
    };
    diag3(6, h->cfg.vel_process_cov);
    diag3(9, h->cfg.acc_bias_process_cov);
    diag3(12, h->cfg.gyr_bias_process_cov);
    diag3(18, h->cfg.imu_acc_process_cov);
    diag3(21, h->cfg.imu_gyr_process_cov);
    diag3(24, h->cfg.kin_bias_process_cov);
    diag3(27, h->cfg.contact_process_cov);
    return lk_set_Q(h, Q.data());
}
int lk_init_process_cov_q(lk_handle* h) {
    CHECK_H(h);
    return init_process_cov_q(h);
}
int lk_set_times(lk_handle* h, uint32_t slot, double last_predict_t, double last_update_t) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    double t[2] = {last_predict_t, last_update_t};
    HIPCHK(h, hipMemcpyAsync(&h->d_filters[slot].last_predict_t, t, sizeof(t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_get_times(lk_handle* h, uint32_t slot, double* last_predict_t, double* last_update_t) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    double t[2];
    HIPCHK(h, hipMemcpyAsync(t, &h->d_filters[slot].last_predict_t, sizeof(t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *last_predict_t = t[0];
    *last_update_t = t[1];
    return LK_OK;
}
int lk_set_acc_norm(lk_handle* h, double acc_norm) {
    CHECK_H(h);
    h->acc_norm = acc_norm;
    return LK_OK;
}
int lk_get_acc_norm(lk_handle* h, double* acc_norm) {
    CHECK_H(h);
    if (!acc_norm) return fail(h, LK_ERR_INVALID, "acc_norm is null");
    *acc_norm = h->acc_norm;
    return LK_OK;
}
int lk_get_fx(lk_handle* h, uint32_t slot, double dt, double* Fx900) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    LAUNCH(h, "fx", hipLaunchKernelGGL(lk_fx_kernel, dim3(1), dim3(64), 0, h->stream, h->d_filters, (int)slot, dt, h->d_tmp,
                                       h->d_tmp + 900));
    HIPCHK(h, hipMemcpyAsync(Fx900, h->d_tmp, sizeof(double) * 900, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_get_function_f(lk_handle* h, uint32_t slot, double dt, double* f30) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    LAUNCH(h, "fx", hipLaunchKernelGGL(lk_fx_kernel, dim3(1), dim3(64), 0, h->stream, h->d_filters, (int)slot, dt, h->d_tmp,
                                       h->d_tmp + 900));
    HIPCHK(h, hipMemcpyAsync(f30, h->d_tmp + 900, sizeof(double) * 30, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_predict(lk_handle* h, uint32_t slot, double dt, int prop_state, int prop_cov) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    LAUNCH(h, "predict_dt", hipLaunchKernelGGL(lk_predict_dt_kernel, dim3(1), dim3(LK_FB), 0, h->stream,
                                               h->d_filters + slot, h->d_Q, dt, prop_state, prop_cov));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_update_by_points(lk_handle* h, uint32_t slot, const double* h6, const double* z, const double* R, size_t N) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    if (N == 0) return LK_OK;
    if (N > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "N exceeds max_scan_points");
    double* d = h->d_rows;
    HIPCHK(h, hipMemcpyAsync(d, h6, sizeof(double) * 6 * N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d + 6 * N, z, sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d + 7 * N, R, sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "obs_points", hipLaunchKernelGGL(lk_obs_points_kernel, dim3(1), dim3(LK_FB), 0, h->stream, h->d_filters,
                                               (int)slot, d, d + 6 * N, d + 7 * N, (int)N));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_update_by_imu(lk_handle* h, uint32_t slot, const double* ki_z6, const double* ki_R6) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    HIPCHK(h, hipMemcpyAsync(h->d_tmp, ki_z6, sizeof(double) * 6, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_tmp + 6, ki_R6, sizeof(double) * 6, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "obs_imu", hipLaunchKernelGGL(lk_obs_imu_kernel, dim3(1), dim3(LK_FB), 0, h->stream, h->d_filters,
                                            (int)slot, h->d_tmp, h->d_tmp + 6));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_update_by_kin_imu(lk_handle* h, uint32_t slot, const double* ki_h, const double* ki_z, const double* ki_R, size_t M) {
    CHECK_H(h);
    CHECK_SLOT(h, slot);
    if (M < 1 || M > 18) return fail(h, LK_ERR_INVALID, "M must be in [1,18]");
    HIPCHK(h, hipMemcpyAsync(h->d_tmp, ki_h, sizeof(double) * 30 * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_tmp + 540, ki_z, sizeof(double) * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_tmp + 560, ki_R, sizeof(double) * M, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "obs_kin", hipLaunchKernelGGL(lk_obs_kin_kernel, dim3(1), dim3(LK_FB), 0, h->stream, h->d_filters, (int)slot,
                                            h->d_tmp, h->d_tmp + 540, h->d_tmp + 560, (int)M));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

}  // extern "C"
extern "C" {

// Ragged batch of SMALL buckets (a real scan: 2 ms time bins of tens of points): the whole bucket chain of a scan - predict,
// residual tiles, update, predict, ... - as ONE WAVE in one launch.  State and covariance stay in LDS from the first
// predict to the last update (WaveSmem), the bucket totals never leave the registers, and there is no launch boundary
// or partial-record round trip per bucket: the batch costs one scan's dependent chain, whatever the number of scans
// (up to the GPU's resident waves).  Arithmetic = residual_tile + wave_update_core + wave_predict_core, i.e. what the
// per-bucket launches of lk_batch_replay_ragged_dev compute; a bucket's tile totals are added in tile order, which is
// the order lk_update_wave_kernel uses for up to 8 tiles (one per group) - the host takes this path only when every bucket
// has <= LK_SCAN_WAVE_MAX points, so both paths give the same bits.
#ifdef LK_DEBUG_PHASES
__device__ unsigned long long lk_sw_dbg[16];   // DEBUG BUILD ONLY: s_memtime deltas per phase of dev_scan_wave, [15] = buckets
#define SW_STAMP(k) do { const unsigned long long t1_ = wall_clock64(); ph_[k] += t1_ - t0_; t0_ = t1_; } while (0)
#else
#define SW_STAMP(k) do { } while (0)
#endif
// RUN (lk_batch_replay_runs_dev; the lk_run_wave kernels below): the slot replays a RUN of consecutive scans on the frozen map, state, covariance and both
// time stamps surviving the scan boundaries as KILO's members do from one KILO::process to the next.  In the CSR tables a run's buckets are one contiguous
// range and their times absolute, so for addressing and time a run IS a scan (rag_nb / rag_t / rag_pt_off through rg.bstart).  Scan-aware are the message
// cursor - behind a scan's last bucket it jumps to the next scan's first record: what a package leaves over is never applied, and at the next scan's first
// bucket every record of ITS package below the bucket's time is (the two rules of rag_bucket()) -, the three per-scan counters, zeroed at the same place,
// and the pose record, written behind the update of a scan's last bucket.  Everything RUN adds is under `if constexpr`: the three kernels without it
// compile to what they were.
extern "C++" {
template <bool RUN = false>
__device__ __forceinline__ void dev_scan_wave(const LkMap& map, const LkParams& pr, LkFilter* filters, const lk_point* __restrict__ pts,
                                              const LkRagged& rg, const double* __restrict__ Q, WaveSmem& sm, double* rows, const int MSG) {
    const bool WITH_IMU = MSG != 0;   // 1: lk_imu messages (only_imu_use), 2: lk_kin_imu messages (leg fusion, KILO.cc:384-390)
    const int slot = blockIdx.x, lane = threadIdx.x;
    LkFilter* f = &filters[slot];
    const int nbk = rag_nb(rg, slot);
    if (nbk == 0) return;
    const double* T = rag_t(rg, slot);
    const unsigned long long* po = rag_pt_off(rg, slot);
    for (int e = lane; e < 900; e += LK_WAVE) sm.P[e] = f->P[e];
    if (lane < 36) sm.x[lane] = f->x[lane];
    double t_upd = f->last_update_t, t_pred = f->last_predict_t;
    unsigned long long n_effect = f->n_effect;
    unsigned int n_updates = f->n_updates, n_buckets = f->n_buckets;
    int last_N = f->last_N, updated = f->updated;
    __syncthreads();
    unsigned int qi = 0, qn = 0;   // this scan's IMU messages (KILO.cc:379-383: those stamped before the bucket come first)
    if constexpr (!RUN)
        if (WITH_IMU) qi = rg.imu_off[slot], qn = rg.imu_off[slot + 1];
    int sc = 0;                // RUN: the scan that owns bucket b ...
    unsigned int b_end = 0u;   // ... and the slot's bucket index behind that scan's last one
    if constexpr (RUN) {
        sc = rag_run_scan(rg, slot, 0);
        b_end = rg.scan_b[sc + 1] - rg.bstart[slot];
        if (WITH_IMU) qi = rg.imu_off[sc], qn = rg.imu_off[sc + 1];
    }
    ResidualOut ro;
    ro.h6 = nullptr, ro.z = nullptr, ro.R = nullptr, ro.valid = nullptr, ro.world = nullptr;
#ifdef LK_DEBUG_PHASES
    unsigned long long ph_[6] = {0, 0, 0, 0, 0, 0}, t0_ = wall_clock64();
#endif
    for (int b = 0; b < nbk;) {
        // next event of the scan: an IMU message stamped before the bucket's time (KILO.cc:379-383), else the bucket
        const double tb_ = T[b];
        const size_t mstride = MSG == 2 ? 33 : 7;
        const bool is_imu = WITH_IMU && qi < qn && rg.imu[mstride * (size_t)qi] < tb_;
        const double t = is_imu ? rg.imu[mstride * (size_t)qi] : tb_;
        SW_STAMP(0);
        wave_predict_core(sm, Q, t - t_upd, t - t_pred, lane, rg.q_diag != 0);   // KILO.cc:111-115 / :240-244
        SW_STAMP(1);
        t_pred = t;
        if (is_imu) {   // predictUpdateImu, KILO.cc:235-258 / predictUpdateKinImu, KILO.cc:260-314
            const double* m = rg.imu + mstride * (size_t)qi;
            if (MSG == 2)
                wave_kin_update_core(sm, rows, m, rg.acc_scale, rg.Rn, rg.kin_noise, lane);
            else
                wave_imu_update_core(sm, m + 1, m + 4, rg.acc_scale, rg.Rn, lane);
            t_upd = t;  // KILO.cc:256 / :312
            ++qi;
            continue;
        }
        const unsigned long long base = po[b];
        const int n = (int)(po[b + 1] - base);
        BucketConst bc;   // load_bucket_const<false> from the LDS-resident state
#pragma unroll
        for (int i = 0; i < 9; ++i) bc.R[i] = sm.x[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) bc.p[i] = sm.x[9 + i];
        {
            const double* P = sm.P;
            bc.Prr = S3{P[0], P[1], P[2], P[31], P[32], P[62]};
            bc.Ppp = S3{P[3 * 30 + 3], P[3 * 30 + 4], P[3 * 30 + 5], P[4 * 30 + 4], P[4 * 30 + 5], P[5 * 30 + 5]};
        }
        double totv = 0.0;  // tot[j] in lanes 0..31
        SW_STAMP(2);
        for (int i0 = 0; i0 < n; i0 += LK_WAVE) {
            __builtin_amdgcn_wave_barrier();  // the previous tile's reads of the rows are complete
            const double a = residual_tile<false, 2, false, true>(map, pr, bc, reinterpret_cast<const float4*>(pts + base), i0 + lane, n, rows, lane, ro, (size_t)0);
            totv += (lane < 29) ? a : 0.0;
        }
        const int N = (int)(lane_bcast<28>(totv) + 0.5);
        SW_STAMP(3);
        n_buckets += 1, last_N = N, updated = N > 0;
        if (N > 0) {
            n_updates += 1, n_effect += (unsigned long long)N;
            t_upd = t;  // KILO.cc:212
            wave_update_core(sm, totv, N, lane);
        }
        SW_STAMP(4);
        __syncthreads();
        ++b;
        if constexpr (RUN) {
            if (rg.bucket_pose)   // (the _cloud entries: the state behind this bucket, updated or not; its time and points read again from the tables - nothing more is kept alive over the update)
                rag_write_bucket(rg.bucket_pose + rg.bstart[slot] + (unsigned int)(b - 1), sm.x, T[b - 1], po[b - 1], (unsigned int)(po[b] - po[b - 1]), (unsigned int)last_N, lane);
            if ((unsigned int)b == b_end) {   // that was the scan's last bucket: its pose, its counters (plain vector stores, as rag_write_pose's)
                lk_pose* p = rg.scan_pose + sc;
                if (lane < 15) reinterpret_cast<double*>(p)[lane] = sm.x[lane];
                if (lane == 0) p->n_effect = n_effect, p->n_buckets = n_buckets, p->n_updates = n_updates;
                if (b < nbk) {   // the next scan (no scan is empty): its own package from the first record on, counters of its own
                    ++sc;
                    b_end = rg.scan_b[sc + 1] - rg.bstart[slot];
                    if (WITH_IMU) qi = rg.imu_off[sc], qn = rg.imu_off[sc + 1];
                    n_effect = 0ull, n_updates = 0u, n_buckets = 0u;
                }
            }
        }
        SW_STAMP(5);
    }
#ifdef LK_DEBUG_PHASES
    if (lane == 0) {
        for (int k = 0; k < 6; ++k) atomicAdd(&lk_sw_dbg[k], ph_[k]);
        atomicAdd(&lk_sw_dbg[15], (unsigned long long)nbk);
    }
#endif
    __syncthreads();
    for (int e = lane; e < 900; e += LK_WAVE) f->P[e] = sm.P[e];
    if (lane < 36) f->x[lane] = sm.x[lane];
    if (lane == 0) {
        f->last_update_t = t_upd, f->last_predict_t = t_pred;
        f->n_effect = n_effect, f->n_updates = n_updates, f->n_buckets = n_buckets, f->last_N = last_N, f->updated = updated;
    }
}
}   // extern "C++"
// Ragged batch WITH insert, the way to bucket b of every scan that has one: the scan's messages stamped before the bucket's time that no
// earlier bucket has consumed (KILO.cc:379-390: predictUpdateImu / predictUpdateKinImu one after the other), then the predict to the bucket's
// time (KILO.cc:111-115) - dev_scan_wave's event loop between two buckets, as a launch of its own (one wave per scan).
__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_rag_advance_kernel(LkFilter* filters, const double* __restrict__ Q, LkRagged rg, int b, int msg_kind) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (b >= rag_nb(rg, slot)) return;
    LkFilter* f = &filters[slot];
    const double* T = rag_t(rg, slot);
    for (int e = lane; e < 900; e += LK_WAVE) sm.P[e] = f->P[e];
    if (lane < 36) sm.x[lane] = f->x[lane];
    double t_upd = f->last_update_t, t_pred = f->last_predict_t;
    __syncthreads();
    const double tb = T[b];
    const LkRagBucket rb = rag_bucket(rg, slot, b, msg_kind != 0);   // (runs: the messages and the look-back are the owning scan's)
    if (msg_kind) {
        const size_t mstride = msg_kind == 2 ? 33 : 7;
        const unsigned int q0 = rb.q0, q1 = rb.q1;
        for (unsigned int q = q0; q < q1; ++q) {
            const double* m = rg.imu + mstride * (size_t)q;
            const double tm = m[0];
            if (!(tm < tb)) break;                  // time-sorted: the rest belongs to later buckets
            if (!rb.first && tm < T[b - 1]) continue;   // consumed on the way to an earlier bucket
            wave_predict_core(sm, Q, tm - t_upd, tm - t_pred, lane, rg.q_diag != 0);
            t_pred = tm;
            if (msg_kind == 2) wave_kin_update_core(sm, rows, m, rg.acc_scale, rg.Rn, rg.kin_noise, lane);
            else wave_imu_update_core(sm, m + 1, m + 4, rg.acc_scale, rg.Rn, lane);
            t_upd = tm;   // KILO.cc:256 / :312
        }
    }
    wave_predict_core(sm, Q, tb - t_upd, tb - t_pred, lane, rg.q_diag != 0);
    t_pred = tb;
    __syncthreads();
    for (int e = lane; e < 900; e += LK_WAVE) f->P[e] = sm.P[e];
    if (lane < 36) f->x[lane] = sm.x[lane];
    if (lane == 0) {
        f->last_update_t = t_upd, f->last_predict_t = t_pred;
        if (rg.run_scan && rb.first) f->n_buckets = 0u, f->n_updates = 0u, f->n_effect = 0ull;   // runs: the update behind this launch counts the scan alone
    }
}


__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_scan_wave_kernel(LkMap map, LkParams pr, LkFilter* filters, const lk_point* __restrict__ pts, LkRagged rg,
                        const double* __restrict__ Q) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    dev_scan_wave(map, pr, filters, pts, rg, Q, sm, rows, 0);
}
__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_scan_wave_imu_kernel(LkMap map, LkParams pr, LkFilter* filters, const lk_point* __restrict__ pts, LkRagged rg,
                            const double* __restrict__ Q) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    dev_scan_wave(map, pr, filters, pts, rg, Q, sm, rows, 1);
}
__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_scan_wave_kin_kernel(LkMap map, LkParams pr, LkFilter* filters, const lk_point* __restrict__ pts, LkRagged rg,
                            const double* __restrict__ Q) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    dev_scan_wave(map, pr, filters, pts, rg, Q, sm, rows, 2);
}
// The same three for runs of scans (dev_scan_wave<true>: lk_batch_replay_runs_dev), one wave per run.
__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_run_wave_kernel(LkMap map, LkParams pr, LkFilter* filters, const lk_point* __restrict__ pts, LkRagged rg,
                       const double* __restrict__ Q) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    dev_scan_wave<true>(map, pr, filters, pts, rg, Q, sm, rows, 0);
}
__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_run_wave_imu_kernel(LkMap map, LkParams pr, LkFilter* filters, const lk_point* __restrict__ pts, LkRagged rg,
                           const double* __restrict__ Q) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    dev_scan_wave<true>(map, pr, filters, pts, rg, Q, sm, rows, 1);
}
__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_run_wave_kin_kernel(LkMap map, LkParams pr, LkFilter* filters, const lk_point* __restrict__ pts, LkRagged rg,
                           const double* __restrict__ Q) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    dev_scan_wave<true>(map, pr, filters, pts, rg, Q, sm, rows, 2);
}
// Runs launch by launch (plain mode with a bucket above LK_SCAN_WAVE_MAX points, or LEGKILO_RAGGED_LEVELS): behind the update of bucket index b
// (lk_update_wave_ragged_kernel, update only) the pose of every scan that ends there - then that slot's three counters are zeroed for the next scan -
// and the predict to the slot's next bucket, which in plain mode is what KILO::process does across a scan boundary as well.
__global__ void __launch_bounds__(LK_WAVE, LK_UPD_WAVES)
    lk_run_tap_predict_kernel(LkFilter* filters, const double* __restrict__ Q, LkRagged rg, int b) {
    __shared__ WaveSmem sm;
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int nbk = rag_nb(rg, slot);
    if (b >= nbk) return;
    LkFilter* f = &filters[slot];
    const LkRagBucket rb = rag_bucket(rg, slot, b, false);
    if (rg.run_scan && rg.bucket_pose) {   // (the _cloud entries: the state the update has left behind this bucket)
        const unsigned long long* po = rag_pt_off(rg, slot);
        rag_write_bucket(rg.bucket_pose + rg.bstart[slot] + (unsigned int)b, f->x, rag_t(rg, slot)[b], po[b], (unsigned int)(po[b + 1] - po[b]), (unsigned int)f->last_N, lane);
    }
    if (rb.pose) {
        rag_write_pose(rb.pose, f->x, f, lane);
        if (lane == 0 && b + 1 < nbk) f->n_buckets = 0u, f->n_updates = 0u, f->n_effect = 0ull;
    }
    if (b + 1 < nbk) dev_update_wave(f, sm, nullptr, 0, 0.0, Q, rag_t(rg, slot)[b + 1], 2);
}

// Registration of replayed runs (the _cloud entries): point i of d_pts under the state behind ITS bucket - x y z as floats, intensity 255 where that bucket
// updated, else 0 (KILO.cc:130-133, :219-223; lk_run_scans_dev's record).  16 B in, 16 B out per point; what has to be found is the point's bucket.  Points
// lie in bucket order and no bucket is empty, so the LK_REG_TILE points of a workgroup from point p0 on lie in the buckets g0 .. g0 + LK_REG_TILE - 1 at
// most, g0 = the bucket of p0: ONE search of the flat pt_off table per workgroup (the same in each of its waves, 64 probes a round), then that window's offsets and - for the
// buckets that do begin inside the tile - the 12 pose doubles and n_effect of their records go to LDS, and every lane searches the window there.
__global__ void __launch_bounds__(LK_REG_TILE)
    lk_register_cloud_kernel(const lk_point* __restrict__ pts, unsigned long long n, const unsigned long long* __restrict__ pt_off, unsigned int B,
                             const lk_bucket_pose* __restrict__ rec, LkParams pr, float* __restrict__ world) {
    typedef float lk_f4v __attribute__((ext_vector_type(4)));
    __shared__ unsigned long long s_off[LK_REG_TILE + 1];
    __shared__ double s_pose[LK_REG_TILE * 12];
    __shared__ unsigned int s_ne[LK_REG_TILE];
    const unsigned int tid = threadIdx.x;
    const unsigned long long p0 = (unsigned long long)blockIdx.x * LK_REG_TILE;
    if (p0 >= n || B == 0u) return;
    const unsigned int np = (unsigned int)((n - p0 < (unsigned long long)LK_REG_TILE) ? n - p0 : (unsigned long long)LK_REG_TILE);
    // (the point itself does not wait for its bucket: its load goes out first)
    lk_f4v p = {0.f, 0.f, 0.f, 0.f};
    if (tid < np) p = __builtin_nontemporal_load(reinterpret_cast<const lk_f4v*>(pts) + p0 + tid);
    // the search, the same in every wave: 64 probes a round, one per lane, at even steps through what is left - offsets increase, so the probes at or below
    // p0 are a prefix and their number names the interval: four dependent loads at 1.5 M buckets where a bisection makes 21
    unsigned int g0 = 0u, hi = B;   // pt_off[g0] <= p0 < pt_off[hi]  (pt_off[0] = 0, pt_off[B] = n)
    while (hi - g0 > 1u) {
        const unsigned int step = (hi - g0 + LK_WAVE - 1) / LK_WAVE;
        const unsigned long long at = (unsigned long long)g0 + (unsigned long long)((tid & (LK_WAVE - 1)) + 1u) * step;
        const unsigned int below = (unsigned int)__popcll(__ballot(at < hi && pt_off[at] <= p0));
        const unsigned long long next = (unsigned long long)g0 + (unsigned long long)(below + 1u) * step;
        g0 += below * step;
        if (next < hi) hi = (unsigned int)next;
    }
    for (unsigned int k = tid; k <= np; k += LK_REG_TILE) s_off[k] = pt_off[(g0 + k < B) ? g0 + k : B];
    __syncthreads();
    // the window's buckets that hold a point of this tile: bucket g0, and those that begin below p0 + np (offsets increase: the count is their number)
    const unsigned int nbw = (unsigned int)__syncthreads_count(tid < np && g0 + tid < B && s_off[tid] < p0 + np);
    for (unsigned int e = tid; e < nbw * 12u; e += LK_REG_TILE) {
        const unsigned int k = e / 12u;
        s_pose[e] = reinterpret_cast<const double*>(rec + g0 + k)[e - 12u * k];   // rot, pos: the record's first 12 doubles
    }
    if (tid < nbw) s_ne[tid] = rec[g0 + tid].n_effect;
    __syncthreads();
    if (tid >= np) return;
    const unsigned long long i = p0 + tid;
    unsigned int lo = 0u, up = nbw;   // s_off[lo] <= i < s_off[up]
    while (up - lo > 1u) {
        const unsigned int mid = (lo + up) >> 1;
        if (s_off[mid] <= i) lo = mid;
        else up = mid;
    }
    BucketConst bc;
#pragma unroll
    for (int j = 0; j < 9; ++j) bc.R[j] = s_pose[12u * lo + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) bc.p[j] = s_pose[12u * lo + 9 + j];
    const V3 w = point_world(p.x, p.y, p.z, bc, pr);
    lk_f4v o;
    o.x = (float)w.x, o.y = (float)w.y, o.z = (float)w.z, o.w = s_ne[lo] ? 255.0f : 0.0f;
    __builtin_nontemporal_store(o, reinterpret_cast<lk_f4v*>(world) + i);
}

// The map as the batch-replay kernels see it: with the dense root grid when it can be built (LkMap::grid).  The grid is derived
// from the hash table + match records and rebuilt when the map has changed since (every mutating entry clears grid_valid);
// building it is two small kernels + a memset, synchronised once - it happens per map snapshot, not per batch.
static constexpr size_t kGridMaxCells = (size_t)1 << 24;   // 16 Mi cells x 144 B = 2.4 GB of grid at most (record INDICES are 32-bit, addressing is 64-bit); larger boxes stay on the hash
int frozen_map(lk_handle* h, LkMap* out) {
    *out = h->map;
    out->grid_on = 0;
    if (!h->grid_enable) return LK_OK;
    if (!h->grid_valid) {
        // the rebuild rewrites the cells (and may move the match pool): nothing enqueued earlier - on any of the handle's streams -
        // may still be reading them
        for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i)
            if (h->side[i]) HIPCHK(h, hipStreamSynchronize(h->side[i]));
        const int init[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
        int mm[6];
        HIPCHK(h, hipMemcpyAsync(h->d_grid_mm, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(lk_grid_bounds_kernel, dim3((h->hash_cap + 255) / 256), dim3(256), 0, h->stream, h->map, h->hash_cap, h->d_grid_mm);
        HIPCHK(h, hipMemcpyAsync(mm, h->d_grid_mm, sizeof(mm), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        LkMap fm = h->map;
        fm.grid_on = 0;
        if (mm[0] <= mm[3]) {
            size_t dim[3], cells = 1;
            bool ok = true;
            for (int c = 0; c < 3; ++c) {
                dim[c] = (size_t)((long long)mm[3 + c] - (long long)mm[c] + 1);
                ok = ok && dim[c] <= kGridMaxCells;
                cells = ok ? cells * dim[c] : cells;
                ok = ok && cells <= kGridMaxCells;
            }
            if (ok && cells > h->grid_cap) {   // grow the match pool: [max_nodes node records | grid cells (+ slack) | flattened subtree lists]
                lk_match_rec* bigger = nullptr;
                const size_t want = cells + cells / 4;
                if (hipMalloc(&bigger, (2 * (size_t)h->map.max_nodes + want) * sizeof(lk_match_rec)) != hipSuccess) {
                    (void)hipGetLastError();   // no room for the grid: stay on the hash table
                    ok = false;
                } else {
                    HIPCHK(h, hipMemcpyAsync(bigger, h->map.match, (size_t)h->map.max_nodes * sizeof(lk_match_rec), hipMemcpyDeviceToDevice, h->stream));
                    HIPCHK(h, hipStreamSynchronize(h->stream));
                    hipFree(h->map.match);
                    std::replace(h->pools.begin(), h->pools.end(), (void*)h->map.match, (void*)bigger);   // the handle owns the new pool instead
                    h->map.match = bigger;
                    h->grid_cap = want;
                    fm.match = bigger;
                }
            }
            if (ok) {
                for (int c = 0; c < 3; ++c) fm.gmin[c] = mm[c], fm.gdim[c] = (int)dim[c];
                fm.grid_base = h->map.max_nodes;
                HIPCHK(h, hipMemsetAsync(fm.match + fm.grid_base, 0xff, cells * sizeof(lk_match_rec), h->stream));
                // the lists (every non-root node at most once) live behind the allocated cells
                const unsigned int cand0 = (unsigned int)((size_t)h->map.max_nodes + h->grid_cap);
                unsigned int* cursor = reinterpret_cast<unsigned int*>(h->d_grid_mm + 6);   // [0] next free list record, [1] overflow flag
                const unsigned int cur0[2] = {cand0, 0u};
                unsigned int cur1[2] = {0u, 0u};
                HIPCHK(h, hipMemcpyAsync(cursor, cur0, sizeof(cur0), hipMemcpyHostToDevice, h->stream));
                hipLaunchKernelGGL(lk_grid_fill_kernel, dim3((h->hash_cap + 255) / 256), dim3(256), 0, h->stream, fm, h->hash_cap, h->pr.max_layer,
                                   cursor, cand0 + h->map.max_nodes);
                HIPCHK(h, hipGetLastError());
                HIPCHK(h, hipMemcpyAsync(cur1, cursor, sizeof(cur1), hipMemcpyDeviceToHost, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));   // the side streams of the replay entries may read it at once
                fm.grid_on = cur1[1] ? 0 : 1;   // list region overflowed (a blob whose subtrees share nodes): this snapshot stays on the hash table
            }
        }
        h->fmap = fm;
        h->grid_valid = true;
        ++h->map_gen;
    }
    *out = h->fmap;
    return LK_OK;
}

// The residual kernel of the uniform batch entries, specialised at compile time for what is launch-uniform: root lookup through
// the frozen-map grid, and ext_R == I (no 3 x 3 extrinsic products, and 18 fewer scalar registers in a kernel whose occupancy
// is set by registers).  LEGKILO_XID=0 keeps the generic instantiation.
using ResidualKernelFn = void (*)(LkMap, LkParams, const LkFilter*, const lk_point*, size_t, int, double*, size_t, ResidualOut, size_t);
static ResidualKernelFn batch_residual_kernel(const lk_handle* h, const LkMap& fmap) {
    if (!fmap.grid_on) return lk_residual_kernel<false, 0, false>;
    return (h->pr.ext_identity && lk_xid_enabled()) ? lk_residual_kernel<false, 1, true> : lk_residual_kernel<false, 1, false>;
}

// Grid of a batch residual launch over `sn` slots x `nblk` tiles: plain 2-D grid (tile, slot); LEGKILO_XCDMAP=1: the XCD-aware 1-D grid of ResidualOut::xmap_slots (A/B)
static dim3 batch_residual_grid(int nblk, int sn, ResidualOut* ro) {
    static const bool xmap = getenv("LEGKILO_XCDMAP") != nullptr && atoi(getenv("LEGKILO_XCDMAP")) != 0;   // measured slower (EXPERIMENTS.md, round 6): off unless asked for
    const unsigned long long wg = 8ull * (unsigned long long)((nblk + 7) / 8) * (unsigned long long)sn;
    if (!xmap || sn < 2 || nblk < 16 || wg >= (1ull << 31)) {
        ro->xmap_slots = 0;
        return dim3(nblk, sn);
    }
    ro->xmap_slots = sn;
    return dim3((unsigned int)wg);
}

__global__ void lk_zero_scan_counters_kernel(LkFilter* filters, unsigned int n_slots) {
    const unsigned int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    LkFilter* f = &filters[s];
    f->n_effect = 0ull, f->n_updates = 0u, f->n_buckets = 0u, f->updated = 0, f->last_N = 0;
}
int zero_scan_counters(lk_handle* h, uint32_t first_slot, uint32_t n_slots) {
    // n_effect, n_updates, n_buckets, updated, last_N of every slot: ONE launch (a 24-byte-wide 2-D memset is two fill kernels)
    hipLaunchKernelGGL(lk_zero_scan_counters_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, h->stream, h->d_filters + first_slot, n_slots);
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}

__global__ void lk_pose_gather_kernel(const LkFilter* filters, lk_pose* out, int n) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const LkFilter* f = &filters[s];
    lk_pose p;
    for (int i = 0; i < 9; ++i) p.rot[i] = f->x[i];
    for (int i = 0; i < 3; ++i) p.pos[i] = f->x[9 + i], p.vel[i] = f->x[12 + i];
    p.n_effect = f->n_effect;
    p.n_buckets = f->n_buckets;
    p.n_updates = f->n_updates;
    out[s] = p;
}
int fetch_poses(lk_handle* h, lk_pose* out, int n) {
    hipLaunchKernelGGL(lk_pose_gather_kernel, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->d_filters, h->d_poses, n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_poses, sizeof(lk_pose) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

// ------------------------------------------------------------------ VoxelMapManager surface
// what lk_map_build and lk_first_frame(_dev) ask before they touch anything: room for the cloud, an empty map
static int map_build_check(lk_handle* h, size_t n) {
    if (n > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "first-frame cloud exceeds max_scan_points");
    unsigned int ctr[LK_CTR_COUNT];
    HIPCHK(h, hipMemcpy(ctr, h->map.counters, sizeof(ctr), hipMemcpyDeviceToHost));
    if (ctr[LK_CTR_NODES] != 0) return fail(h, LK_ERR_STATE, "lk_map_build needs an empty map (BuildVoxelMap runs once)");
    return LK_OK;
}
// BuildVoxelMap from the two clouds in HBM (n x 3 floats each, rot / covariances of slot 0): the core of lk_map_build and lk_first_frame(_dev)
static int map_build_dev(lk_handle* h, const float* d_w, const float* d_b, size_t n) {
    h->grid_valid = false;
    lk_pt_rec* d_bpts = nullptr;
    unsigned int *d_k0 = nullptr, *d_k1 = nullptr;
    int *d_i0 = nullptr, *d_i1 = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    DevTemps tmp;
    HIPCHK(h, tmp.alloc(&d_bpts, sizeof(lk_pt_rec) * n));
    HIPCHK(h, tmp.alloc(&d_k0, sizeof(unsigned int) * n));
    HIPCHK(h, tmp.alloc(&d_k1, sizeof(unsigned int) * n));
    HIPCHK(h, tmp.alloc(&d_i0, sizeof(int) * n));
    HIPCHK(h, tmp.alloc(&d_i1, sizeof(int) * n));
    hipLaunchKernelGGL(lk_bucket_begin_kernel, dim3(1), dim3(256), 0, h->stream, h->map);
    const int nb = (int)((n + 255) / 256);
    LAUNCH(h, "build_points", hipLaunchKernelGGL(lk_build_points_kernel, dim3(nb), dim3(256), 0, h->stream, h->map, h->pr,
                                                 h->d_filters, d_w, d_b, (int)n, d_bpts, d_k0, d_i0));
    // stable sort by root id: groups each root's points, preserving input order (voxel_map.cc:313-332)
    HIPCHK(h, lk_prim_sort_pairs(nullptr, tmp_bytes, d_k0, d_k1, d_i0, d_i1, n, 0, 32, h->stream));
    HIPCHK(h, tmp.alloc(&d_tmp, tmp_bytes));
    HIPCHK(h, lk_prim_sort_pairs(d_tmp, tmp_bytes, d_k0, d_k1, d_i0, d_i1, n, 0, 32, h->stream));
    LAUNCH(h, "build_segments",
           hipLaunchKernelGGL(lk_build_segments_kernel, dim3(nb), dim3(256), 0, h->stream, h->map, d_k1, (int)n));
    int grid = std::min(std::max((int)((n + 3) / 4), 1), 256);
    LAUNCH(h, "build_tree", hipLaunchKernelGGL(lk_build_tree_kernel, dim3(grid), dim3(LK_MB), 0, h->stream, h->map, h->pr,
                                               d_bpts, d_i1, d_i0));
    return check_map_errors(h);  // synchronises the stream; `tmp` frees the temporaries
}
int lk_map_build(lk_handle* h, const float* xyz_world, const float* xyz_body, size_t n) {
    CHECK_H(h);
    if (n == 0) return LK_OK;
    LKCHK(map_build_check(h, n));
    float *d_w = nullptr, *d_b = nullptr;
    DevTemps tmp;
    HIPCHK(h, tmp.alloc(&d_w, sizeof(float) * 3 * n));
    HIPCHK(h, tmp.alloc(&d_b, sizeof(float) * 3 * n));
    HIPCHK(h, hipMemcpyAsync(d_w, xyz_world, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_b, xyz_body, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
    return map_build_dev(h, d_w, d_b, n);   // synchronises the stream before `tmp` frees the clouds
}

// ------------------------------------------------------------------ first frame (KILO.cc:332-352; lk_pre_kernels.h, lk_ff_*)
// The raw cloud and the first package's messages are in HBM: state initialisation (one lane), cloudLidarToWorld (one thread per point),
// BuildVoxelMap from the two clouds where they lie, then acc_norm_ and the two time stamps.
static int first_frame_check(lk_handle* h, const void* raw, size_t n, int msg_kind, const void* msgs, size_t n_msg) {
    if (n == 0 || n_msg == 0) return fail(h, LK_ERR_INVALID, "Data packet is not ready: the first frame needs a cloud and at least one message (KILO.cc:326-329)");
    if (msg_kind != MSG_IMU && msg_kind != MSG_KIN) return fail(h, LK_ERR_INVALID, "msg_kind must be 1 (lk_imu) or 2 (lk_kin_imu)");
    if (!raw || !msgs) return fail(h, LK_ERR_INVALID, "null argument");
    if (n_msg >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "more than 2^31 messages");
    return map_build_check(h, n);
}
static int first_frame_dev(lk_handle* h, const lk_point* d_raw, size_t n, double end_time, int msg_kind, const void* d_msgs, size_t n_msg) {
    float *d_w = nullptr, *d_b = nullptr;
    double* d_norm = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        d_norm = c.take<double>(1);
        d_w = c.take<float>(3 * n), d_b = c.take<float>(3 * n);
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->ff, bytes));
    carve(h->ff.p);
    LKCHK(init_process_cov_q(h));
    const unsigned int stride = (unsigned int)msg_record_bytes(msg_kind);
    const unsigned int acc_off = msg_kind == MSG_KIN ? offsetof(lk_kin_imu, acc) : offsetof(lk_imu, acc);
    static_assert(offsetof(lk_imu, gyr) == offsetof(lk_imu, acc) + 24 && offsetof(lk_kin_imu, gyr) == offsetof(lk_kin_imu, acc) + 24, "gyr lies behind acc");
    LAUNCH(h, "ff_init", hipLaunchKernelGGL(lk_ff_init_kernel, dim3(1), dim3(256), 0, h->stream, h->d_filters, static_cast<const unsigned char*>(d_msgs),
                                            (unsigned int)n_msg, stride, acc_off, h->cfg.gravity, end_time, d_norm));
    LAUNCH(h, "ff_world", hipLaunchKernelGGL(lk_ff_world_kernel, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_filters, h->pr, d_raw,
                                             (int)n, d_w, d_b));
    LKCHK(map_build_dev(h, d_w, d_b, n));
    double acc_norm = 0.0;
    HIPCHK(h, hipMemcpyAsync(&acc_norm, d_norm, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->acc_norm = acc_norm;   // KILO.cc:349
    return LK_OK;
}
int lk_first_frame_dev(lk_handle* h, const lk_point* d_raw, size_t n, double end_time, int msg_kind, const void* d_msgs, size_t n_msg) {
    CHECK_H(h);
    LKCHK(first_frame_check(h, d_raw, n, msg_kind, d_msgs, n_msg));
    return first_frame_dev(h, d_raw, n, end_time, msg_kind, d_msgs, n_msg);
}
int lk_first_frame(lk_handle* h, const lk_point* raw, size_t n, double end_time, int msg_kind, const void* msgs, size_t n_msg) {
    CHECK_H(h);
    LKCHK(first_frame_check(h, raw, n, msg_kind, msgs, n_msg));
    const size_t msg_bytes = n_msg * msg_record_bytes(msg_kind);
    lk_point* d_raw = nullptr;
    unsigned char* d_msgs = nullptr;
    DevTemps tmp;
    HIPCHK(h, tmp.alloc(&d_raw, sizeof(lk_point) * n));
    HIPCHK(h, tmp.alloc(&d_msgs, msg_bytes));
    HIPCHK(h, hipMemcpyAsync(d_raw, raw, sizeof(lk_point) * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_msgs, msgs, msg_bytes, hipMemcpyHostToDevice, h->stream));
    const int rc = first_frame_dev(h, d_raw, n, end_time, msg_kind, d_msgs, n_msg);
    if (rc != LK_OK) hipStreamSynchronize(h->stream);   // (the temporaries are freed on return)
    return rc;
}

int lk_map_update(lk_handle* h, const double* pw, const double* var9, size_t n) {
    CHECK_H(h);
    if (n == 0) return LK_OK;
    if (n > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "n exceeds max_scan_points");
    h->grid_valid = false;
    std::vector<lk_pt_rec> st(n);
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) st[i].pw[c] = pw[3 * i + c];
        const double* v = var9 + 9 * i;
        st[i].var[0] = v[0], st[i].var[1] = v[1], st[i].var[2] = v[2], st[i].var[3] = v[4], st[i].var[4] = v[5], st[i].var[5] = v[8];
    }
    lk_pt_rec* d_pv = nullptr;
    DevTemps tmp;
    HIPCHK(h, tmp.alloc(&d_pv, sizeof(lk_pt_rec) * n));
    HIPCHK(h, hipMemcpyAsync(d_pv, st.data(), sizeof(lk_pt_rec) * n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(lk_bucket_begin_kernel, dim3(1), dim3(256), 0, h->stream, h->map);
    const int nb = (int)((n + 255) / 256);
    LAUNCH(h, "queue_pv", hipLaunchKernelGGL(lk_queue_pv_kernel, dim3(nb), dim3(256), 0, h->stream, h->map, h->pr, d_pv, (int)n));
    int grid = std::min(std::max((int)((n + 3) / 4), 1), 256);
    LAUNCH(h, "insert_pv_root", hipLaunchKernelGGL(lk_insert_root_kernel<true>, dim3(grid), dim3(LK_MB), 0, h->stream, h->map, h->pr,
                                                   h->d_filters, (const lk_point*)nullptr, d_pv, (int)n));
    LAUNCH(h, "insert_pv", hipLaunchKernelGGL(lk_insert_apply_kernel<true>, dim3(grid), dim3(LK_MB), 0, h->stream, h->map, h->pr,
                                              h->d_filters, (const lk_point*)nullptr, d_pv, (int)n));
    LAUNCH(h, "insert_pv_fallback", hipLaunchKernelGGL(lk_insert_fallback_kernel<true>, dim3(std::min(grid, 8)), dim3(LK_MB), 0, h->stream,
                                                       h->map, h->pr, h->d_filters, (const lk_point*)nullptr, d_pv, (int)n));
    return check_map_errors(h);  // synchronises the stream; `tmp` frees d_pv
}

int upload_xyz_as_points(lk_handle* h, const float* xyz, size_t n) {
    std::vector<lk_point> p(n);
    for (size_t i = 0; i < n; ++i) p[i] = lk_point{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f};
    HIPCHK(h, hipMemcpyAsync(h->d_scan, p.data(), sizeof(lk_point) * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // p goes out of scope
    return LK_OK;
}

int lk_residuals(lk_handle* h, const float* xyz_body, size_t n, double* h6, double* z, double* R, uint8_t* valid) {
    CHECK_H(h);
    if (n == 0) return LK_OK;
    if (n > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "n exceeds max_scan_points");
    int rc = upload_xyz_as_points(h, xyz_body, n);
    if (rc) return rc;
    ResidualOut ro;
    ro.h6 = h->d_rows;
    ro.z = h->d_rows + 6 * n;
    ro.R = h->d_rows + 7 * n;
    ro.valid = h->d_valid;
    ro.world = nullptr;
    const int nblk = (int)((n + LK_RB - 1) / LK_RB);
    LAUNCH(h, "residual_rows",
           hipLaunchKernelGGL(lk_residual_kernel<true>, dim3(nblk, 1), dim3(LK_RB), 0, h->stream, h->map, h->pr, h->d_filters,
                              h->d_scan, (size_t)0, (int)n, h->d_partials, h->part_stride, ro, (size_t)0));
    HIPCHK(h, hipMemcpyAsync(h6, ro.h6, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(z, ro.z, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(R, ro.R, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(valid, ro.valid, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

// VoxelMapManager::build_single_residual (voxel_map.cc:363-427) for n caller-held pointWithVar: see lk_query_kernels.h
int lk_match_points(lk_handle* h, size_t n, const int32_t* keys3, const double* pw, const double* var9, uint8_t* found, uint8_t* success,
                    double* prob, double* normal3, double* center3, double* d, float* dis_to_plane, int32_t* layer) {
    CHECK_H(h);
    if (n == 0) return LK_OK;
    if (!keys3 || !pw || !var9 || !found || !success || !prob || !normal3 || !center3 || !d || !dis_to_plane || !layer)
        return fail(h, LK_ERR_INVALID, "lk_match_points: null argument");
    if (n > (size_t)INT_MAX / 9) return fail(h, LK_ERR_INVALID, "lk_match_points: n too large");
    int rc = join_side_streams(h);   // the map as every earlier call on this handle left it
    if (rc) return rc;
    // one device buffer for the inputs and outputs of a query, kept by the handle and grown on demand (a caller of the class surface may ask point by point)
    double *d_pw = nullptr, *d_var = nullptr, *d_f64 = nullptr;
    int *d_keys = nullptr, *d_layer = nullptr;
    float* d_dis = nullptr;
    unsigned char* d_u8 = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        d_pw = c.take<double>(3 * n), d_var = c.take<double>(9 * n);
        d_f64 = c.take<double>(8 * n);   // prob | normal | center | d
        d_keys = c.take<int>(3 * n), d_layer = c.take<int>(n);
        d_dis = c.take<float>(n);
        d_u8 = c.take<unsigned char>(2 * n);   // found | success
        return c.total();
    };
    const size_t need = carve(nullptr);
    LKCHK(reserve(h, h->query, need, std::max(need + need / 2, (size_t)65536) - need));
    carve(h->query.p);
    HIPCHK(h, hipMemcpyAsync(d_keys, keys3, sizeof(int) * 3 * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_pw, pw, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_var, var9, sizeof(double) * 9 * n, hipMemcpyHostToDevice, h->stream));
    LkMatchOut mo;
    mo.found = d_u8, mo.success = d_u8 + n;
    mo.prob = d_f64, mo.normal = d_f64 + n, mo.center = d_f64 + 4 * n, mo.d = d_f64 + 7 * n;
    mo.dis_to_plane = d_dis, mo.layer = d_layer;
    LAUNCH(h, "match_points", hipLaunchKernelGGL(lk_match_points_kernel, dim3((unsigned int)((n + 63) / 64)), dim3(64), 0, h->stream, h->map, h->pr,
                                                 (const int*)d_keys, (const double*)d_pw, (const double*)d_var, (int)n, mo));
    HIPCHK(h, hipMemcpyAsync(found, mo.found, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(success, mo.success, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(prob, mo.prob, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(normal3, mo.normal, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(center3, mo.center, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(d, mo.d, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(dis_to_plane, mo.dis_to_plane, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(layer, mo.layer, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

// clearMemOutOfMap (voxel_map.cc:571-594) as a pool compaction; see lk_map_kernels.h.  The steps (MapCompact, lk_internal.h) are shared with
// lk_overlay_commit.
__global__ void lk_validate_ids_kernel(LkMap map, unsigned int n_nodes, unsigned int n_blocks, unsigned int hash_cap);
int compact_begin(lk_handle* h, MapCompact* mc, unsigned int x_nodes, unsigned int x_blocks, unsigned int x_roots) {
    unsigned int ctr[LK_CTR_COUNT];
    HIPCHK(h, hipMemcpyAsync(ctr, h->map.counters, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    mc->n_nodes = std::min(ctr[LK_CTR_NODES], h->map.max_nodes), mc->n_blocks = std::min(ctr[LK_CTR_BLOCKS], h->map.max_blocks), mc->n_roots = ctr[LK_CTR_ROOTS];
    mc->x_nodes = x_nodes, mc->x_blocks = x_blocks, mc->x_roots = x_roots;
    if (mc->n_roots + x_roots == 0) return LK_OK;   // nothing to compact: no scratch
    const size_t N = (size_t)mc->n_nodes + x_nodes, B = std::max<size_t>((size_t)mc->n_blocks + x_blocks, 1);
    const auto flags = [&](void* base) {   // one allocation, one memset
        LkCarve c(base);
        mc->alive_node = c.take<unsigned int>(N), mc->alive_block = c.take<unsigned int>(B), mc->drop = c.take<unsigned int>(std::max(mc->n_nodes, 1u));
        mc->cnt = c.take<unsigned int>(4);
        return c.total();
    };
    const auto ranks = [&](void* base) {
        LkCarve c(base);
        mc->new_node = c.take<unsigned int>(N), mc->new_block = c.take<unsigned int>(B);
        return c.total();
    };
    void *fb = nullptr, *rb = nullptr;
    const size_t fbytes = flags(nullptr);
    if (mc->tmp.alloc(&fb, fbytes) != hipSuccess || mc->tmp.alloc(&rb, ranks(nullptr)) != hipSuccess ||
        mc->tmp.alloc(&mc->kept, sizeof(lk_root_rec) * ((size_t)mc->n_roots + x_roots)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, LK_ERR_HIP, "map compaction: out of device memory");
    }
    flags(fb), ranks(rb);
    HIPCHK(h, hipMemsetAsync(fb, 0, fbytes, h->stream));
    return LK_OK;
}
int compact_mark(lk_handle* h, MapCompact* mc, const LkSlideBox& box, bool with_drop) {
    hipLaunchKernelGGL(lk_slide_mark_kernel, dim3((h->hash_cap + 255) / 256), dim3(256), 0, h->stream, h->map, box, h->hash_cap,
                       mc->alive_node, mc->alive_block, mc->kept, mc->cnt, with_drop ? mc->drop : nullptr);
    HIPCHK(h, hipGetLastError());
    unsigned int hc[2];
    HIPCHK(h, hipMemcpyAsync(hc, mc->cnt, sizeof(hc), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hc[0] + hc[1] != mc->n_roots) return fail(h, LK_ERR_STATE, "hash table and root counter disagree");
    mc->kept_roots = hc[0], mc->removed_roots = hc[1];
    return LK_OK;
}
int compact_count(lk_handle* h, MapCompact* mc) {   // dense new ids
    const size_t N = (size_t)mc->n_nodes + mc->x_nodes, B = (size_t)mc->n_blocks + mc->x_blocks;
    size_t t1 = 0, t2 = 0;
    HIPCHK(h, lk_prim_exclusive_scan(nullptr, t1, mc->alive_node, mc->new_node, N, h->stream));
    HIPCHK(h, lk_prim_exclusive_scan(nullptr, t2, mc->alive_block, mc->new_block, std::max<size_t>(B, 1), h->stream));
    LKCHK(reserve(h, h->prim_tmp, std::max(t1, t2)));
    t1 = t2 = h->prim_tmp.cap;
    HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, t1, mc->alive_node, mc->new_node, N, h->stream));
    if (B) HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, t2, mc->alive_block, mc->new_block, B, h->stream));
    unsigned int last[6] = {0, 0, 0, 0, 0, 0};  // new_node[N-1], alive_node[N-1], new_block[B-1], alive_block[B-1]; new_node / new_block at the second pool's first record
    HIPCHK(h, hipMemcpyAsync(&last[0], mc->new_node + N - 1, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&last[1], mc->alive_node + N - 1, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    if (B) {
        HIPCHK(h, hipMemcpyAsync(&last[2], mc->new_block + B - 1, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&last[3], mc->alive_block + B - 1, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    }
    if (mc->x_nodes) HIPCHK(h, hipMemcpyAsync(&last[4], mc->new_node + mc->n_nodes, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    if (mc->x_blocks) HIPCHK(h, hipMemcpyAsync(&last[5], mc->new_block + mc->n_blocks, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    mc->all_nodes = last[0] + last[1], mc->all_blocks = last[2] + last[3];
    mc->live_nodes = mc->x_nodes ? last[4] : mc->all_nodes, mc->live_blocks = mc->x_blocks ? last[5] : mc->all_blocks;
    return LK_OK;
}
int compact_move(lk_handle* h, MapCompact* mc) {
    h->grid_valid = false;
    const unsigned int live_nodes = mc->live_nodes, live_blocks = mc->live_blocks;
    lk_node_rec* tn = nullptr;
    lk_plane_rec* tp = nullptr;
    lk_match_rec* tm = nullptr;
    lk_block_rec* tb = nullptr;
    if (mc->tmp.alloc(&tn, sizeof(lk_node_rec) * std::max(live_nodes, 1u)) != hipSuccess || mc->tmp.alloc(&tp, sizeof(lk_plane_rec) * std::max(live_nodes, 1u)) != hipSuccess ||
        mc->tmp.alloc(&tm, sizeof(lk_match_rec) * std::max(live_nodes, 1u)) != hipSuccess || mc->tmp.alloc(&tb, sizeof(lk_block_rec) * std::max(live_blocks, 1u)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, LK_ERR_HIP, "map compaction: out of device memory");
    }
    if (mc->n_nodes)
        hipLaunchKernelGGL(lk_slide_move_nodes_kernel, dim3((mc->n_nodes + 255) / 256), dim3(256), 0, h->stream, h->map, mc->n_nodes, mc->alive_node,
                           mc->new_node, mc->new_block, tn, tp, tm, 0);
    if (mc->n_blocks)
        hipLaunchKernelGGL(lk_slide_move_blocks_kernel, dim3(mc->n_blocks), dim3(64), 0, h->stream, h->map, mc->alive_block, mc->new_block, tb);
    HIPCHK(h, hipGetLastError());
    if (live_nodes) {
        HIPCHK(h, hipMemcpyAsync(h->map.nodes, tn, sizeof(lk_node_rec) * live_nodes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->map.planes, tp, sizeof(lk_plane_rec) * live_nodes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->map.match, tm, sizeof(lk_match_rec) * live_nodes, hipMemcpyDeviceToDevice, h->stream));
    }
    if (live_blocks)
        HIPCHK(h, hipMemcpyAsync(h->map.blocks, tb, sizeof(lk_block_rec) * live_blocks, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(lk_slide_hash_clear_kernel, dim3((h->hash_cap + 255) / 256), dim3(256), 0, h->stream, h->map, h->hash_cap);
    if (mc->kept_roots)
        hipLaunchKernelGGL(lk_slide_remap_roots_kernel, dim3((mc->kept_roots + 255) / 256), dim3(256), 0, h->stream, mc->kept, mc->kept_roots, mc->new_node);
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}
int compact_finish(lk_handle* h, MapCompact* mc, unsigned int n_nodes, unsigned int n_blocks, unsigned int n_roots, bool validate_ids) {
    if (n_roots)
        hipLaunchKernelGGL(lk_hash_insert_kernel, dim3((n_roots + 255) / 256), dim3(256), 0, h->stream, h->map, h->pr, mc->kept, (int)n_roots);
    hipLaunchKernelGGL(lk_slide_counters_kernel, dim3(1), dim3(1), 0, h->stream, h->map, n_nodes, n_blocks, n_roots);
    if (validate_ids) {   // as lk_map_import_dev: a dangling id is an error now, not a walk later
        const unsigned int nv = std::max(n_nodes, h->hash_cap);
        hipLaunchKernelGGL(lk_validate_ids_kernel, dim3((nv + 255) / 256), dim3(256), 0, h->stream, h->map, n_nodes, n_blocks, h->hash_cap);
    }
    HIPCHK(h, hipGetLastError());
    return check_map_errors(h);  // synchronises: the scratch buffers may be released after this
}
static int clear_outside(lk_handle* h, const LkSlideBox& box, uint32_t* n_removed) {
    if (n_removed) *n_removed = 0;
    h->grid_valid = false;
    MapCompact mc;
    LKCHK(compact_begin(h, &mc, 0, 0, 0));
    if (mc.n_roots == 0) return LK_OK;
    LKCHK(compact_mark(h, &mc, box, false));
    if (n_removed) *n_removed = mc.removed_roots;
    if (mc.removed_roots == 0) return LK_OK;
    LKCHK(compact_count(h, &mc));
    LKCHK(compact_move(h, &mc));
    return compact_finish(h, &mc, mc.live_nodes, mc.live_blocks, mc.kept_roots, false);
}

int lk_map_clear_outside(lk_handle* h, int32_t x_max, int32_t x_min, int32_t y_max, int32_t y_min, int32_t z_max, int32_t z_min,
                         uint32_t* n_removed) {
    CHECK_H(h);
    return clear_outside(h, LkSlideBox{x_max, x_min, y_max, y_min, z_max, z_min}, n_removed);
}

int lk_map_slide(lk_handle* h, const double* position, double sliding_thresh, int32_t half_map_size, int32_t* slid, uint32_t* n_removed) {
    CHECK_H(h);
    if (!position) return fail(h, LK_ERR_INVALID, "position is null");
    if (slid) *slid = 0;
    if (n_removed) *n_removed = 0;
    const double dx = position[0] - h->last_slide_position[0], dy = position[1] - h->last_slide_position[1],
                 dz = position[2] - h->last_slide_position[2];
    if (sqrt(dx * dx + dy * dy + dz * dz) < sliding_thresh) return LK_OK;  // voxel_map.cc:553
    for (int i = 0; i < 3; ++i) h->last_slide_position[i] = position[i];
    const double vs = h->cfg.max_voxel_size;  // the DOUBLE voxel size (voxel_map.cc:561)
    const int ix = (int)floor(position[0] / vs), iy = (int)floor(position[1] / vs), iz = (int)floor(position[2] / vs);
    if (slid) *slid = 1;
    return clear_outside(h, LkSlideBox{ix + half_map_size, ix - half_map_size, iy + half_map_size, iy - half_map_size, iz + half_map_size,
                                       iz - half_map_size}, n_removed);
}

int lk_map_slide_position(lk_handle* h, int32_t set, double* last3) {
    CHECK_H(h);
    if (!last3) return fail(h, LK_ERR_INVALID, "last3 is null");
    for (int i = 0; i < 3; ++i) {
        if (set) h->last_slide_position[i] = last3[i];
        else last3[i] = h->last_slide_position[i];
    }
    return LK_OK;
}

int lk_map_stats(lk_handle* h, uint32_t* n_roots, uint32_t* n_nodes, uint32_t* n_blocks) {
    CHECK_H(h);
    unsigned int ctr[LK_CTR_COUNT];
    HIPCHK(h, hipMemcpyAsync(ctr, h->map.counters, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_roots) *n_roots = ctr[LK_CTR_ROOTS];
    if (n_nodes) *n_nodes = ctr[LK_CTR_NODES];
    if (n_blocks) *n_blocks = ctr[LK_CTR_BLOCKS];
    return LK_OK;
}

static void fill_header(lk_handle* h, lk_blob_header& hd, const unsigned int* ctr, uint32_t version) {
    memset(&hd, 0, sizeof(hd));
    hd.magic = LK_BLOB_MAGIC;
    hd.version = version;
    hd.n_roots = ctr[LK_CTR_ROOTS];
    hd.n_nodes = std::min(ctr[LK_CTR_NODES], h->map.max_nodes);
    hd.n_blocks = std::min(ctr[LK_CTR_BLOCKS], h->map.max_blocks);
    hd.block_pts = LK_BLOCK_PTS;
    hd.voxel_size = h->cfg.max_voxel_size;
    hd.max_layer = h->cfg.max_layer;
    hd.max_points_num = h->cfg.max_points_num;
}

// host blob of one LkMap (the handle's map, or one slot's overlay): header | roots (sorted by key) | nodes | planes | blocks
int export_map_blob(lk_handle* h, const LkMap& m, unsigned int hash_cap, void* blob, size_t* bytes) {
    if (!bytes) return fail(h, LK_ERR_INVALID, "bytes is null");
    unsigned int ctr[LK_CTR_COUNT];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(ctr, m.counters, sizeof(ctr), hipMemcpyDeviceToHost));
    lk_blob_header hd;
    fill_header(h, hd, ctr, LK_ABI_VERSION);
    hd.n_nodes = std::min(ctr[LK_CTR_NODES], m.max_nodes);
    hd.n_blocks = std::min(ctr[LK_CTR_BLOCKS], m.max_blocks);
    size_t total = sizeof(hd) + (size_t)hd.n_roots * sizeof(lk_root_rec) + (size_t)hd.n_nodes * (sizeof(lk_node_rec) + sizeof(lk_plane_rec)) +
                   (size_t)hd.n_blocks * sizeof(lk_block_rec);
    hd.bytes = total;
    if (!blob) {
        *bytes = total;
        return LK_OK;
    }
    if (*bytes < total) return fail(h, LK_ERR_INVALID, "blob buffer too small");
    std::vector<int4> table(hash_cap);
    HIPCHK(h, hipMemcpy(table.data(), m.hash, sizeof(int4) * hash_cap, hipMemcpyDeviceToHost));
    std::vector<lk_root_rec> roots;
    roots.reserve(hd.n_roots);
    for (const int4& e : table)
        if (e.w >= 0) roots.push_back(lk_root_rec{{e.x, e.y, e.z}, e.w});
    if (roots.size() != hd.n_roots) return fail(h, LK_ERR_STATE, "hash table and root counter disagree");
    std::sort(roots.begin(), roots.end(), [](const lk_root_rec& a, const lk_root_rec& b) {
        return std::lexicographical_compare(a.key, a.key + 3, b.key, b.key + 3);
    });
    char* p = (char*)blob;
    memcpy(p, &hd, sizeof(hd));
    p += sizeof(hd);
    memcpy(p, roots.data(), roots.size() * sizeof(lk_root_rec));
    p += roots.size() * sizeof(lk_root_rec);
    HIPCHK(h, hipMemcpy(p, m.nodes, (size_t)hd.n_nodes * sizeof(lk_node_rec), hipMemcpyDeviceToHost));
    p += (size_t)hd.n_nodes * sizeof(lk_node_rec);
    HIPCHK(h, hipMemcpy(p, m.planes, (size_t)hd.n_nodes * sizeof(lk_plane_rec), hipMemcpyDeviceToHost));
    p += (size_t)hd.n_nodes * sizeof(lk_plane_rec);
    HIPCHK(h, hipMemcpy(p, m.blocks, (size_t)hd.n_blocks * sizeof(lk_block_rec), hipMemcpyDeviceToHost));
    *bytes = total;
    return LK_OK;
}
int lk_map_export(lk_handle* h, void* blob, size_t* bytes) {
    CHECK_H(h);
    return export_map_blob(h, h->map, h->hash_cap, blob, bytes);
}
// the voxels scan `slot` of the last overlay replay holds privately (the roots its inserts touched or created), as a map blob: the
// slot's key table is turned into the int4 form the exporter reads (entry index = root node id)


// A blob is only usable by a handle configured like the one that wrote it: the voxel size defines the keys, max_layer
// and max_points_num the insert state machine.
static int check_blob_config(lk_handle* h, const lk_blob_header& hd) {
    if (hd.voxel_size != h->cfg.max_voxel_size || hd.max_layer != h->cfg.max_layer || hd.max_points_num != h->cfg.max_points_num) {
        char buf[200];
        snprintf(buf, sizeof(buf), "blob was written with voxel_size %.9g / max_layer %d / max_points_num %d, the handle has %.9g / %d / %d",
                 hd.voxel_size, hd.max_layer, hd.max_points_num, h->cfg.max_voxel_size, h->cfg.max_layer, h->cfg.max_points_num);
        return fail(h, LK_ERR_INVALID, buf);
    }
    return LK_OK;
}

// child / block / root-node ids of an imported map must index the imported pools (device-resident blobs are checked
// where they are; a host blob is checked on the host before anything is copied)
__global__ void lk_validate_ids_kernel(LkMap map, unsigned int n_nodes, unsigned int n_blocks, unsigned int hash_cap) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n_nodes) {
        const lk_node_rec* nd = &map.nodes[i];
#pragma unroll
        for (int c = 0; c < 8; ++c) bad |= nd->child[c] < -1 || nd->child[c] >= (int)n_nodes;
        bad |= nd->block < -1 || nd->block >= (int)n_blocks;
        bad |= nd->npts < 0 || (nd->block >= 0 && nd->npts > LK_BLOCK_PTS);
    }
    if (i < hash_cap) {
        const int4 e = map.hash[i];
        bad |= e.w >= (int)n_nodes || e.w < LK_LOCKED;
    }
    if (bad) atomicOr(&map.counters[LK_CTR_ERR], LK_E_BAD_BLOB);
}

static int reset_pools(lk_handle* h) {
    h->grid_valid = false;
    unsigned int ninit = std::max(h->hash_cap, h->map.max_nodes);
    hipLaunchKernelGGL(lk_pool_init_kernel, dim3((ninit + 255) / 256), dim3(256), 0, h->stream, h->map, h->hash_cap);
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}

int lk_map_import(lk_handle* h, const void* blob, size_t bytes) {
    CHECK_H(h);
    if (!blob || bytes < sizeof(lk_blob_header)) return fail(h, LK_ERR_INVALID, "blob too small");
    lk_blob_header hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != LK_BLOB_MAGIC || hd.version != LK_ABI_VERSION || hd.block_pts != LK_BLOCK_PTS || hd.bytes > bytes)
        return fail(h, LK_ERR_INVALID, "bad blob header");
    {   // the counts must account for every byte: a truncated or corrupt blob must not make the copies read past `blob`
        const size_t expect = sizeof(hd) + (size_t)hd.n_roots * sizeof(lk_root_rec) +
                              (size_t)hd.n_nodes * (sizeof(lk_node_rec) + sizeof(lk_plane_rec)) + (size_t)hd.n_blocks * sizeof(lk_block_rec);
        if (expect != hd.bytes) return fail(h, LK_ERR_INVALID, "blob size does not match its record counts (truncated or corrupt)");
    }
    int rc = check_blob_config(h, hd);
    if (rc) return rc;
    if (hd.n_nodes > h->map.max_nodes || hd.n_blocks > h->map.max_blocks || 2 * (size_t)hd.n_roots > h->hash_cap)
        return fail(h, LK_ERR_CAPACITY, "blob exceeds pool capacities");
    {   // ids are range-checked here, on the host copy, before the device sees them
        const char* q = (const char*)blob + sizeof(hd);
        const lk_root_rec* rr = (const lk_root_rec*)q;
        for (uint32_t i = 0; i < hd.n_roots; ++i)
            if (rr[i].node < 0 || (uint32_t)rr[i].node >= hd.n_nodes) return fail(h, LK_ERR_INVALID, "blob: root node id out of range");
        const lk_node_rec* nn = (const lk_node_rec*)(q + (size_t)hd.n_roots * sizeof(lk_root_rec));
        for (uint32_t i = 0; i < hd.n_nodes; ++i) {
            lk_node_rec nd;
            memcpy(&nd, &nn[i], sizeof(nd));
            for (int c = 0; c < 8; ++c)
                if (nd.child[c] < -1 || nd.child[c] >= (int)hd.n_nodes) return fail(h, LK_ERR_INVALID, "blob: child id out of range");
            if (nd.block < -1 || nd.block >= (int)hd.n_blocks || nd.npts < 0 || (nd.block >= 0 && nd.npts > LK_BLOCK_PTS))
                return fail(h, LK_ERR_INVALID, "blob: point block id / count out of range");
        }
    }
    rc = reset_pools(h);
    if (rc) return rc;
    const char* p = (const char*)blob + sizeof(hd);
    lk_root_rec* d_roots = nullptr;
    DevTemps tmp;
    if (hd.n_roots) {
        HIPCHK(h, tmp.alloc(&d_roots, sizeof(lk_root_rec) * hd.n_roots));
        HIPCHK(h, hipMemcpyAsync(d_roots, p, sizeof(lk_root_rec) * hd.n_roots, hipMemcpyHostToDevice, h->stream));
    }
    p += (size_t)hd.n_roots * sizeof(lk_root_rec);
    HIPCHK(h, hipMemcpyAsync(h->map.nodes, p, (size_t)hd.n_nodes * sizeof(lk_node_rec), hipMemcpyHostToDevice, h->stream));
    p += (size_t)hd.n_nodes * sizeof(lk_node_rec);
    HIPCHK(h, hipMemcpyAsync(h->map.planes, p, (size_t)hd.n_nodes * sizeof(lk_plane_rec), hipMemcpyHostToDevice, h->stream));
    p += (size_t)hd.n_nodes * sizeof(lk_plane_rec);
    HIPCHK(h, hipMemcpyAsync(h->map.blocks, p, (size_t)hd.n_blocks * sizeof(lk_block_rec), hipMemcpyHostToDevice, h->stream));
    if (hd.n_roots)
        hipLaunchKernelGGL(lk_hash_insert_kernel, dim3((hd.n_roots + 255) / 256), dim3(256), 0, h->stream, h->map, h->pr,
                           d_roots, (int)hd.n_roots);
    if (hd.n_nodes)
        hipLaunchKernelGGL(lk_derive_match_kernel, dim3((hd.n_nodes + 255) / 256), dim3(256), 0, h->stream, h->map, (int)hd.n_nodes);
    unsigned int ctr[LK_CTR_COUNT] = {0};
    ctr[LK_CTR_NODES] = hd.n_nodes, ctr[LK_CTR_BLOCKS] = hd.n_blocks, ctr[LK_CTR_ROOTS] = hd.n_roots;
    // only the first three counters: the hash-insert kernel may raise the error word concurrently
    HIPCHK(h, hipMemcpyAsync(h->map.counters, ctr, 3 * sizeof(unsigned int), hipMemcpyHostToDevice, h->stream));
    return check_map_errors(h);
}

// Device-resident blob for the RCCL broadcast: header | hash table (full) | nodes | planes | blocks (used prefixes).
// version carries bit 0x100 to distinguish it from the host blob.
int lk_map_export_dev(lk_handle* h, void* d_blob, size_t* bytes) {
    CHECK_H(h);
    if (!bytes) return fail(h, LK_ERR_INVALID, "bytes is null");
    unsigned int ctr[LK_CTR_COUNT];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(ctr, h->map.counters, sizeof(ctr), hipMemcpyDeviceToHost));
    lk_blob_header hd;
    fill_header(h, hd, ctr, LK_ABI_VERSION | 0x100u);
    size_t total = sizeof(hd) + sizeof(int4) * (size_t)h->hash_cap + (size_t)hd.n_nodes * (sizeof(lk_node_rec) + sizeof(lk_plane_rec)) +
                   (size_t)hd.n_blocks * sizeof(lk_block_rec);
    total = (total + 255) & ~(size_t)255;
    hd.bytes = total;
    if (!d_blob) {
        *bytes = total;
        return LK_OK;
    }
    if (*bytes < total) return fail(h, LK_ERR_INVALID, "device blob buffer too small");
    char* p = (char*)d_blob;
    HIPCHK(h, hipMemcpyAsync(p, &hd, sizeof(hd), hipMemcpyHostToDevice, h->stream));
    p += sizeof(hd);
    HIPCHK(h, hipMemcpyAsync(p, h->map.hash, sizeof(int4) * (size_t)h->hash_cap, hipMemcpyDeviceToDevice, h->stream));
    p += sizeof(int4) * (size_t)h->hash_cap;
    HIPCHK(h, hipMemcpyAsync(p, h->map.nodes, (size_t)hd.n_nodes * sizeof(lk_node_rec), hipMemcpyDeviceToDevice, h->stream));
    p += (size_t)hd.n_nodes * sizeof(lk_node_rec);
    HIPCHK(h, hipMemcpyAsync(p, h->map.planes, (size_t)hd.n_nodes * sizeof(lk_plane_rec), hipMemcpyDeviceToDevice, h->stream));
    p += (size_t)hd.n_nodes * sizeof(lk_plane_rec);
    HIPCHK(h, hipMemcpyAsync(p, h->map.blocks, (size_t)hd.n_blocks * sizeof(lk_block_rec), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *bytes = total;
    return LK_OK;
}

int lk_map_import_dev(lk_handle* h, const void* d_blob, size_t bytes) {
    CHECK_H(h);
    if (!d_blob || bytes < sizeof(lk_blob_header)) return fail(h, LK_ERR_INVALID, "device blob too small");
    lk_blob_header hd;
    HIPCHK(h, hipMemcpy(&hd, d_blob, sizeof(hd), hipMemcpyDeviceToHost));
    if (hd.magic != LK_BLOB_MAGIC || hd.version != (LK_ABI_VERSION | 0x100u) || hd.bytes > bytes)
        return fail(h, LK_ERR_INVALID, "bad device blob header");
    int rc = check_blob_config(h, hd);
    if (rc) return rc;
    if (hd.n_nodes > h->map.max_nodes || hd.n_blocks > h->map.max_blocks)
        return fail(h, LK_ERR_CAPACITY, "device blob exceeds pool capacities");
    size_t expect = sizeof(hd) + sizeof(int4) * (size_t)h->hash_cap + (size_t)hd.n_nodes * (sizeof(lk_node_rec) + sizeof(lk_plane_rec)) +
                    (size_t)hd.n_blocks * sizeof(lk_block_rec);
    if (((expect + 255) & ~(size_t)255) != hd.bytes)
        return fail(h, LK_ERR_INVALID, "device blob was exported with different capacities (max_roots must match)");
    rc = reset_pools(h);
    if (rc) return rc;
    const char* p = (const char*)d_blob + sizeof(hd);
    HIPCHK(h, hipMemcpyAsync(h->map.hash, p, sizeof(int4) * (size_t)h->hash_cap, hipMemcpyDeviceToDevice, h->stream));
    p += sizeof(int4) * (size_t)h->hash_cap;
    HIPCHK(h, hipMemcpyAsync(h->map.nodes, p, (size_t)hd.n_nodes * sizeof(lk_node_rec), hipMemcpyDeviceToDevice, h->stream));
    p += (size_t)hd.n_nodes * sizeof(lk_node_rec);
    HIPCHK(h, hipMemcpyAsync(h->map.planes, p, (size_t)hd.n_nodes * sizeof(lk_plane_rec), hipMemcpyDeviceToDevice, h->stream));
    p += (size_t)hd.n_nodes * sizeof(lk_plane_rec);
    HIPCHK(h, hipMemcpyAsync(h->map.blocks, p, (size_t)hd.n_blocks * sizeof(lk_block_rec), hipMemcpyDeviceToDevice, h->stream));
    if (hd.n_nodes)
        hipLaunchKernelGGL(lk_derive_match_kernel, dim3((hd.n_nodes + 255) / 256), dim3(256), 0, h->stream, h->map, (int)hd.n_nodes);
    unsigned int ctr[LK_CTR_COUNT] = {0};
    ctr[LK_CTR_NODES] = hd.n_nodes, ctr[LK_CTR_BLOCKS] = hd.n_blocks, ctr[LK_CTR_ROOTS] = hd.n_roots;
    HIPCHK(h, hipMemcpyAsync(h->map.counters, ctr, sizeof(ctr), hipMemcpyHostToDevice, h->stream));
    {
        const unsigned int nv = std::max(hd.n_nodes, h->hash_cap);
        hipLaunchKernelGGL(lk_validate_ids_kernel, dim3((nv + 255) / 256), dim3(256), 0, h->stream, h->map, hd.n_nodes, hd.n_blocks, h->hash_cap);
        HIPCHK(h, hipGetLastError());
    }
    rc = check_map_errors(h);
    if (rc) {  // a map with dangling ids must not stay loaded
        reset_pools(h);
        hipStreamSynchronize(h->stream);
        return fail(h, LK_ERR_INVALID, "device blob: node / block ids out of range");
    }
    return LK_OK;
}

// ------------------------------------------------------------------ the lidar front end: sensor decode, voxel-grid centroid filter + time sort (lk_pre_kernels.h)
// One body in two stages over the S messages / scans of a call: front_decode (keep flags, compaction, scatter) and front_grid (bounds, cell keys, cell
// sort, cells, centroids, time sort, gather).  lk_decode_scan_dev is the first at S = 1, lk_preprocess_scan_dev the second at S = 1 on the caller's
// points, lk_decode_scans_dev both.  Host round trips per call, none per message: one after the decode (per-message decoded counts and raw times), one
// after the centroids (per-scan overflow words and cell offsets: the time sort's size) and one at the end.  Both sorts are stable and stay inside a
// scan (lk_prim_sort_pairs_in_segments, a segment per scan), so ties keep the input order whatever S is.
namespace {
struct FrontPool {   // the per-call view of h->pre
    unsigned int *flags, *pos, *sid, *k0, *k1, *v0, *v1;   // sid: null with one scan, and so are msg_off / pt_off (the kernels' "everything is scan 0")
    int* starts;
    lk_point *dec, *cells;
    unsigned long long* msg_off;
    unsigned int *pt_off, *dec_off, *err, *cell_off, *misc;
    int* mm;
    double* first_last;
    lk_point* io_out;        // the host wrappers' device copies: the cloud that goes back ...
    unsigned char* io_in;    // ... and what came up (raw lk_points or message bytes); the device entries carve none
};
// carves the arrays for P points of S messages out of `base` (nullptr: only counts) and returns the bytes they take; the host wrappers' staging arrays
// come last, so that the device entry's view of the same buffer is the same but for them
size_t front_carve(void* base, size_t P, size_t S, size_t n_io, size_t in_bytes, FrontPool& d) {
    LkCarve c(base, 256);
    d.flags = c.take<unsigned int>(P), d.pos = c.take<unsigned int>(P);
    d.sid = S > 1 ? c.take<unsigned int>(P) : nullptr;
    d.k0 = c.take<unsigned int>(P), d.k1 = c.take<unsigned int>(P), d.v0 = c.take<unsigned int>(P), d.v1 = c.take<unsigned int>(P);
    d.starts = c.take<int>(P);
    d.dec = c.take<lk_point>(P), d.cells = c.take<lk_point>(P);
    d.msg_off = S > 1 ? c.take<unsigned long long>(S) : nullptr;
    d.pt_off = S > 1 ? c.take<unsigned int>(S + 1) : nullptr;
    // dec_off [S + 1] | mm [6 S] | err [S] | cell_off [S + 1] taken as ONE array: lk_preprocess_scan_dev writes the first three with one copy, err | cell_off are read back with one
    d.dec_off = c.take<unsigned int>(9 * S + 2);
    d.mm = base ? reinterpret_cast<int*>(d.dec_off + S + 1) : nullptr;
    d.err = base ? d.dec_off + 7 * S + 1 : nullptr, d.cell_off = base ? d.err + S : nullptr;
    d.misc = c.take<unsigned int>(8);
    d.first_last = c.take<double>(2 * S);
    d.io_out = c.take<lk_point>(n_io), d.io_in = c.take<unsigned char>(in_bytes);
    return c.total();
}
}  // namespace
// The arrays are laid out for the call's P and S: a wrapper that hands a staging array to a device entry passes the same P and S on, so both see the same
// layout.  A call of ONE message grows the buffer ahead (a live stream's scans differ a little in size).  The rocPRIM temporary storage is sized
// for P as well (every sort and scan of the call runs over at most P elements).
static int front_reserve(lk_handle* h, size_t P, size_t S, size_t n_io, size_t in_bytes, FrontPool& d) {
    const size_t need = front_carve(nullptr, P, S, n_io, in_bytes, d), G = P + P / 4 + 1024;
    LKCHK(reserve(h, h->pre, need, S == 1 ? front_carve(nullptr, G, 1, n_io ? G : 0, in_bytes / P * G, d) - need : 0));
    front_carve(h->pre.p, P, S, n_io, in_bytes, d);
    size_t t1 = 0, t2 = 0;
    HIPCHK(h, lk_prim_exclusive_scan(nullptr, t1, d.flags, d.pos, P, h->stream));
    HIPCHK(h, lk_prim_sort_pairs_in_segments(nullptr, t2, d.k0, d.k1, d.v0, d.v1, (unsigned int)P, (unsigned int)S, d.dec_off, d.dec_off + 1, 0, 32, h->stream));
    return reserve(h, h->prim_tmp, std::max(t1, t2));
}

// decode stage: the kept points of S messages (P raw points in all; S > 1: d.msg_off / d.pt_off are on their way, base = the buffer they count from; one
// message: base = its first byte) into `out`, in input order.  Leaves dec_off, the raw first / last times and every scan's initial bounds / overflow
// word on the device and brings dec_off [S + 1] and first_last [2 S] to the host.  label: the prefix of the launches' profile names
static int front_decode(lk_handle* h, const char* label, const FrontPool& d, const unsigned char* base, size_t S, size_t P, const LkDecodeArgs& a,
                        lk_point* out, unsigned int* dec_off, double* first_last) {
    const std::string L(label);
    const unsigned int n = (unsigned int)P, nb = (n + 255) / 256;
    LAUNCH(h, (L + "flags").c_str(), hipLaunchKernelGGL(lk_dscan_flags_kernel, dim3(nb), dim3(256), 0, h->stream, base, d.msg_off, d.pt_off, (int)S, n, a, d.flags));
    size_t tb = h->prim_tmp.cap;
    HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, tb, d.flags, d.pos, P, h->stream));
    LAUNCH(h, (L + "scatter").c_str(), hipLaunchKernelGGL(lk_dscan_scatter_kernel, dim3(nb), dim3(256), 0, h->stream, base, d.msg_off, d.pt_off, (int)S, n, a,
                                                          d.flags, d.pos, out, d.sid, d.dec_off, d.first_last, d.mm, d.err));
    HIPCHK(h, hipMemcpyAsync(dec_off, d.dec_off, 4 * (S + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(first_last, d.first_last, 8 * 2 * S, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

// grid stage: D points of S scans (scan s = [dec_off[s], dec_off[s + 1]) on the device, with sid, initial bounds and overflow words) -> per-scan bounds and
// cell keys, a stable sort by cell inside each scan, cells (a new one at every scan boundary), centroids, the scans' offsets over the cells (cell_off
// [S + 1], to the host), a stable sort by time inside each scan's cells, the gather into d_out.  who: names the entry and the message in the overflow
// refusal (null: the bare text of the one-scan entries)
static int front_grid(lk_handle* h, const char* label, const char* who, const FrontPool& d, const lk_point* pts, unsigned int D, size_t S, float leaf,
                      lk_point* d_out, unsigned int* cell_off) {
    const std::string L(label);
    const unsigned int Si = (unsigned int)S, db = (D + 255) / 256;
    const float inv = 1.0f / leaf;  // inverse_leaf_size_, float as in PCL
    const unsigned int gy = S == 1 ? std::min(db, 1024u) : std::min(64u, std::max(1u, D / Si / 2048u));   // (the bounds' atomics are order-free)
    LAUNCH(h, (L + "minmax").c_str(), hipLaunchKernelGGL(lk_dscan_minmax_kernel, dim3(Si, gy), dim3(256), 0, h->stream, pts, d.dec_off, d.mm));
    LAUNCH(h, (L + "cellidx").c_str(), hipLaunchKernelGGL(lk_dscan_cellidx_kernel, dim3(db), dim3(256), 0, h->stream, pts, D, inv, d.mm, d.sid, d.k0, d.v0, d.err));
    size_t tb = h->prim_tmp.cap;
    HIPCHK(h, lk_prim_sort_pairs_in_segments(h->prim_tmp.p, tb, d.k0, d.k1, d.v0, d.v1, D, Si, d.dec_off, d.dec_off + 1, 0, 32, h->stream));
    LAUNCH(h, (L + "heads").c_str(), hipLaunchKernelGGL(lk_dscan_heads_kernel, dim3(db), dim3(256), 0, h->stream, d.k1, d.sid, D, d.flags));
    tb = h->prim_tmp.cap;
    HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, tb, d.flags, d.pos, D, h->stream));
    // one scan: its offsets over the cells are { 0, cells } - the starts kernel writes the total there itself, and the launch of the offsets is saved
    unsigned int* ncells_d = S == 1 ? d.cell_off + 1 : d.misc;
    LAUNCH(h, (L + "starts").c_str(), hipLaunchKernelGGL(lk_pre_starts_kernel, dim3(db), dim3(256), 0, h->stream, d.flags, d.pos, (int)D, d.starts, ncells_d));
    LAUNCH(h, (L + "centroid").c_str(), hipLaunchKernelGGL(lk_pre_centroid_kernel, dim3(db), dim3(256), 0, h->stream, pts, (const int*)d.v1, d.starts, ncells_d,
                                                           (int)D, d.cells, d.k0, (int*)d.v0));
    if (S > 1)
        LAUNCH(h, (L + "celloff").c_str(), hipLaunchKernelGGL(lk_dscan_celloff_kernel, dim3((Si + 1 + 255) / 256), dim3(256), 0, h->stream, d.dec_off, d.pos, ncells_d,
                                                              (int)S, d.cell_off));
    std::vector<unsigned int> ec(2 * S + 1);   // err [S] | cell_off [S + 1]
    HIPCHK(h, hipMemcpyAsync(ec.data(), d.err, 4 * (2 * S + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (S == 1) ec[1] = 0u;
    for (size_t s = 0; s < S; ++s)
        if (ec[s])
            return fail(h, LK_ERR_INVALID, (who ? std::string(who) + ": message " + std::to_string(s) + ": " : std::string()) +
                                               "voxel grid leaf too small for the cloud extent (index overflow)");
    const unsigned int Cn = ec[2 * S];
    tb = h->prim_tmp.cap;
    HIPCHK(h, lk_prim_sort_pairs_in_segments(h->prim_tmp.p, tb, d.k0, d.k1, d.v0, d.v1, Cn, Si, d.cell_off, d.cell_off + 1, 0, 32, h->stream));
    LAUNCH(h, (L + "gather").c_str(), hipLaunchKernelGGL(lk_pre_gather_kernel, dim3((Cn + 255) / 256), dim3(256), 0, h->stream, d.cells, (const int*)d.v1, (int)Cn,
                                                         d_out));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::copy(ec.begin() + S, ec.end(), cell_off);
    return LK_OK;
}

// what lk_decode_scan(s)_dev refuse in a point layout (nullptr: none)
static const char* cloud_layout_error(const lk_cloud_layout* layout) {
    if (layout->lidar_type < 1 || layout->lidar_type > 3) return "lidar_type must be 1, 2 or 3";
    const uint32_t tsz = layout->lidar_type == 3 ? 8u : 4u;
    if (layout->off_x + 4 > layout->point_step || layout->off_y + 4 > layout->point_step || layout->off_z + 4 > layout->point_step ||
        layout->off_time + tsz > layout->point_step)
        return "field offsets exceed point_step";
    return nullptr;
}

int lk_decode_scan_dev(lk_handle* h, const void* d_msg, size_t n_points, const lk_cloud_layout* layout, double time_scale,
                       int filter_num, float blind, double header_stamp, lk_point* d_out, size_t* n_out, double* begin_time,
                       double* end_time) {
    CHECK_H(h);
    if (!d_msg || !layout || !d_out || !n_out || n_points == 0 || filter_num < 1 || n_points > 0x7fffffffu)
        return fail(h, LK_ERR_INVALID, "lk_decode_scan: bad argument");
    if (const char* e = cloud_layout_error(layout)) return fail(h, LK_ERR_INVALID, e);
    FrontPool d;
    LKCHK(front_reserve(h, n_points, 1, 0, 0, d));
    LkDecodeArgs a;
    a.lay = *layout, a.time_scale = time_scale, a.filter_num = filter_num, a.blind = blind;
    unsigned int dec_off[2] = {0, 0};
    double tfl[2] = {0, 0};
    LKCHK(front_decode(h, "decode_", d, (const unsigned char*)d_msg, 1, n_points, a, d_out, dec_off, tfl));
    *n_out = dec_off[1];
    const double base = layout->lidar_type == 3 ? 0.0 : header_stamp;  // lidar_processing.cc:34-35,63-64 vs :91-92
    if (begin_time) *begin_time = base + tfl[0];
    if (end_time) *end_time = base + tfl[1];
    return LK_OK;
}

int lk_decode_scan(lk_handle* h, const void* msg, size_t n_points, const lk_cloud_layout* layout, double time_scale, int filter_num,
                   float blind, double header_stamp, lk_point* out, size_t* n_out, double* begin_time, double* end_time) {
    CHECK_H(h);
    if (!msg || !layout || !out || n_points == 0) return fail(h, LK_ERR_INVALID, "lk_decode_scan: bad argument");
    const size_t bytes = n_points * (size_t)layout->point_step;
    FrontPool d;
    LKCHK(front_reserve(h, n_points, 1, n_points, bytes, d));
    HIPCHK(h, hipMemcpyAsync(d.io_in, msg, bytes, hipMemcpyHostToDevice, h->stream));
    LKCHK(lk_decode_scan_dev(h, d.io_in, n_points, layout, time_scale, filter_num, blind, header_stamp, d.io_out, n_out, begin_time, end_time));
    HIPCHK(h, hipMemcpyAsync(out, d.io_out, sizeof(lk_point) * (*n_out), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

int lk_preprocess_scan_dev(lk_handle* h, const lk_point* d_raw, size_t n_raw, float leaf, lk_point* d_out, size_t* n_out) {
    CHECK_H(h);
    if (!d_raw || !d_out || !n_out || n_raw == 0 || !(leaf > 0.f)) return fail(h, LK_ERR_INVALID, "lk_preprocess_scan: bad argument");
    if (n_raw > 0x7fffffffu) return fail(h, LK_ERR_INVALID, "too many points");
    FrontPool d;
    LKCHK(front_reserve(h, n_raw, 1, 0, 0, d));
    // what the decode stage leaves behind for a scan: dec_off = { 0, n } | the initial bounds | the overflow word
    const unsigned int init[9] = {0u, (unsigned int)n_raw, 0x7fffffffu, 0x7fffffffu, 0x7fffffffu, 0x80000000u, 0x80000000u, 0x80000000u, 0u};
    HIPCHK(h, hipMemcpyAsync(d.dec_off, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    unsigned int cell_off[2] = {0, 0};
    LKCHK(front_grid(h, "pre_", nullptr, d, d_raw, (unsigned int)n_raw, 1, leaf, d_out, cell_off));
    *n_out = cell_off[1];
    return LK_OK;
}

int lk_decode_scans_dev(lk_handle* h, const void* d_msgs, size_t n_msgs, const uint64_t* msg_off, const uint32_t* n_points,
                        const double* header_stamp, const lk_cloud_layout* layout, double time_scale, int filter_num, float blind,
                        float leaf, lk_point* d_out, uint64_t* scan_off, double* t_begin, double* t_end) {
    CHECK_H(h);
    if (!d_msgs || n_msgs == 0 || !msg_off || !n_points || !header_stamp || !layout || !d_out || !scan_off || filter_num < 1 || !(leaf > 0.f))
        return fail(h, LK_ERR_INVALID, "lk_decode_scans_dev: bad argument");
    if (n_msgs > 0x7fffffffu) return fail(h, LK_ERR_INVALID, "lk_decode_scans_dev: too many messages");
    if (const char* e = cloud_layout_error(layout)) return fail(h, LK_ERR_INVALID, e);
    const size_t S = n_msgs;
    std::vector<unsigned int> pt_off(S + 1);
    size_t P = 0;
    for (size_t s = 0; s < S; ++s) {
        if (n_points[s] == 0) return fail(h, LK_ERR_INVALID, "lk_decode_scans_dev: message " + std::to_string(s) + " has no points");
        if (s && header_stamp[s] < header_stamp[s - 1])   // lidarCallBack's time check (ros_interface.cc)
            return fail(h, LK_ERR_INVALID, "lk_decode_scans_dev: message " + std::to_string(s) + ": header stamp older than message " +
                                               std::to_string(s - 1) + "'s");
        pt_off[s] = (unsigned int)P;
        P += n_points[s];
        if (P > 0x7fffffffu)
            return fail(h, LK_ERR_INVALID, "lk_decode_scans_dev: more than 0x7fffffff points from message " + std::to_string(s) + " on: split the run");
    }
    pt_off[S] = (unsigned int)P;
    FrontPool d;
    LKCHK(front_reserve(h, P, S, 0, 0, d));
    LkDecodeArgs a;
    a.lay = *layout, a.time_scale = time_scale, a.filter_num = filter_num, a.blind = blind;
    const unsigned char* base = (const unsigned char*)d_msgs;
    if (S > 1) {
        HIPCHK(h, hipMemcpyAsync(d.msg_off, msg_off, 8 * S, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d.pt_off, pt_off.data(), 4 * (S + 1), hipMemcpyHostToDevice, h->stream));
    } else {
        base += msg_off[0];
    }
    std::vector<unsigned int> dec_off(S + 1), cell_off(S + 1);
    std::vector<double> fl(2 * S);
    LKCHK(front_decode(h, "dscan_", d, base, S, P, a, d.dec, dec_off.data(), fl.data()));
    for (size_t s = 0; s < S; ++s)
        if (dec_off[s + 1] == dec_off[s])
            return fail(h, LK_ERR_INVALID, "lk_decode_scans_dev: message " + std::to_string(s) + " decodes to no points (filter_num / blind)");
    LKCHK(front_grid(h, "dscan_", "lk_decode_scans_dev", d, d.dec, dec_off[S], S, leaf, d_out, cell_off.data()));
    for (size_t s = 0; s <= S; ++s) scan_off[s] = cell_off[s];
    for (size_t s = 0; s < S; ++s) {
        const double b = layout->lidar_type == 3 ? 0.0 : header_stamp[s];  // lidar_processing.cc:34-35,63-64 vs :91-92
        if (t_begin) t_begin[s] = b + fl[2 * s];
        if (t_end) t_end[s] = b + fl[2 * s + 1];
    }
    return LK_OK;
}

// ------------------------------------------------------------------ map clouds: the voxel grid over files of registered points (lk_mapcloud_kernels.h)
// Two host round trips per call, none per file: after the per-file grids (status and overflow words: a bad file is refused before the sort) and at
// the end (the files' cell offsets).  The sort is rocPRIM's stable segmented radix sort with a segment per file - ties keep the input order, which is
// the order of the sums; a single file goes through the device-wide stable sort instead (a segment is sorted by ONE workgroup).
namespace {
struct MclPool {   // the per-call view of h->mcl
    unsigned int *k0, *k1, *v0, *v1;   // keys / indices before and after the sort; k0 / v0 hold the head flags and their ranks afterwards
    int* starts;
    float4* sorted;
    unsigned int *file_off, *cell_off, *status, *misc;
    int *mm, *grid;
    float4 *io_in, *io_out;            // lk_downsample_clouds' device copies (n_io records each; the device entry carves none)
};
// carves the arrays for N points of F files out of `base` (nullptr: only counts) and returns the bytes they take; the host entry's staging arrays
// come last, so that the device entry's view of the same buffer is the same but for them
size_t mcl_carve(void* base, size_t N, size_t F, size_t n_io, MclPool& d) {
    LkCarve c(base, 256);
    d.k0 = c.take<unsigned int>(N), d.k1 = c.take<unsigned int>(N), d.v0 = c.take<unsigned int>(N), d.v1 = c.take<unsigned int>(N);
    d.starts = c.take<int>(N);
    d.sorted = c.take<float4>(N);
    d.file_off = c.take<unsigned int>(F + 1), d.cell_off = c.take<unsigned int>(F + 1);
    d.status = c.take<unsigned int>(F);
    d.misc = c.take<unsigned int>(8);
    d.mm = c.take<int>(6 * F);
    d.grid = c.take<int>(LK_MC_GRID_WORDS * F);
    d.io_in = c.take<float4>(n_io), d.io_out = c.take<float4>(n_io);
    return c.total();
}
}  // namespace

static int mcl_reserve(lk_handle* h, size_t N, size_t F, size_t n_io, MclPool& d) {
    LKCHK(reserve(h, h->mcl, mcl_carve(nullptr, N, F, n_io, d)));
    mcl_carve(h->mcl.p, N, F, n_io, d);
    size_t t1 = 0, t2 = 0;
    HIPCHK(h, lk_prim_exclusive_scan(nullptr, t1, d.k0, d.v0, N, h->stream));
    HIPCHK(h, lk_prim_sort_pairs_in_segments(nullptr, t2, d.k0, d.k1, d.v0, d.v1, (unsigned int)N, (unsigned int)F, d.file_off, d.file_off + 1, 0, 31, h->stream));
    return reserve(h, h->prim_tmp, std::max(t1, t2));
}

// what both entries refuse before anything is launched; *n_pts: file_off[n_files] - file_off[0]
static int mcl_check_tables(lk_handle* h, const char* who, const void* in, size_t n_files, const uint64_t* file_off, float leaf, const void* out,
                            const uint64_t* out_off, size_t* n_pts) {
    const std::string w = std::string(who) + ": ";
    if (!in || !file_off || !out || !out_off) return fail(h, LK_ERR_INVALID, w + "null argument");
    if (n_files == 0) return fail(h, LK_ERR_INVALID, w + "n_files is 0");
    if (!std::isfinite(leaf) || !(leaf > 0.f)) return fail(h, LK_ERR_INVALID, w + "leaf must be finite and above 0");
    if (((uintptr_t)in & 15u) || ((uintptr_t)out & 15u)) return fail(h, LK_ERR_INVALID, w + "the input and output clouds must be 16-byte aligned");
    for (size_t f = 0; f < n_files; ++f) {
        if (file_off[f + 1] < file_off[f]) return fail(h, LK_ERR_INVALID, w + "file_off decreases at file " + std::to_string(f));
        if (file_off[f + 1] == file_off[f]) return fail(h, LK_ERR_INVALID, w + "file " + std::to_string(f) + " is empty");
        if (file_off[f + 1] - file_off[0] > 0x7fffffffull)
            return fail(h, LK_ERR_INVALID, w + "more than 0x7fffffff points from file " + std::to_string(f) + " on: split the call");
    }
    *n_pts = (size_t)(file_off[n_files] - file_off[0]);
    const uintptr_t a = (uintptr_t)in + 16u * (uintptr_t)file_off[0], b = (uintptr_t)out, len = 16u * (uintptr_t)*n_pts;
    if (a < b + len && b < a + len) return fail(h, LK_ERR_INVALID, w + "the output overlaps the input");
    return LK_OK;
}

int lk_downsample_clouds_dev(lk_handle* h, const float* d_world, size_t n_files, const uint64_t* file_off, float leaf, float* d_out, uint64_t* out_off,
                             uint8_t* unfiltered) {
    CHECK_H(h);
    size_t N = 0;
    LKCHK(mcl_check_tables(h, "lk_downsample_clouds_dev", d_world, n_files, file_off, leaf, d_out, out_off, &N));
    const size_t F = n_files;
    MclPool d;
    LKCHK(mcl_reserve(h, N, F, 0, d));
    std::vector<unsigned int> foff(F + 1);
    size_t biggest = 0;
    for (size_t f = 0; f <= F; ++f) foff[f] = (unsigned int)(file_off[f] - file_off[0]);
    for (size_t f = 0; f < F; ++f) biggest = std::max(biggest, (size_t)(foff[f + 1] - foff[f]));
    const float4* pts = reinterpret_cast<const float4*>(d_world) + file_off[0];
    const unsigned int n = (unsigned int)N, nb = (n + 255) / 256, Fi = (unsigned int)F, fb = (Fi + 255) / 256;
    const float inv = 1.0f / leaf;  // inverse_leaf_size_, float as in PCL
    HIPCHK(h, hipMemcpyAsync(d.file_off, foff.data(), 4 * (F + 1), hipMemcpyHostToDevice, h->stream));
    // 1. per-file bounds with the non-finite / range words, the files' grids
    const unsigned int gy = bounds_rows(F, biggest);
    LAUNCH(h, "mc_init", hipLaunchKernelGGL(lk_mc_init_kernel, dim3(fb), dim3(256), 0, h->stream, d.mm, d.status, (int)Fi));
    LAUNCH(h, "mc_bounds", hipLaunchKernelGGL(lk_mc_bounds_kernel, dim3(Fi, gy), dim3(256), 0, h->stream, pts, d.file_off, inv, d.mm, d.status));
    LAUNCH(h, "mc_grid", hipLaunchKernelGGL(lk_mc_grid_kernel, dim3(fb), dim3(256), 0, h->stream, d.mm, d.status, inv, (int)Fi, d.grid));
    std::vector<int> grid(LK_MC_GRID_WORDS * F);
    HIPCHK(h, hipMemcpyAsync(grid.data(), d.grid, sizeof(int) * grid.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t f = 0; f < F; ++f)
        if (const int st = grid[LK_MC_GRID_WORDS * f + 7])
            return fail(h, LK_ERR_INVALID, "lk_downsample_clouds_dev: file " + std::to_string(f) +
                                               ((st & LK_MC_BAD_NONFINITE) ? " holds a coordinate that is not finite" : " holds a coordinate with |p / leaf| >= 2^30"));
    // 2. a cell key per point, a stable sort by key inside each file, cells (a new one at every file boundary), their first points
    LAUNCH(h, "mc_keys", hipLaunchKernelGGL(lk_mc_keys_kernel, dim3(nb), dim3(256), 0, h->stream, pts, n, d.file_off, (int)Fi, inv, d.grid, d.k0, d.v0));
    size_t tb = h->prim_tmp.cap;
    HIPCHK(h, lk_prim_sort_pairs_in_segments(h->prim_tmp.p, tb, d.k0, d.k1, d.v0, d.v1, n, Fi, d.file_off, d.file_off + 1, 0, 31, h->stream));
    unsigned int *flags = d.k0, *pos = d.v0, *ncells_d = d.misc;
    LAUNCH(h, "mc_heads", hipLaunchKernelGGL(lk_mc_heads_kernel, dim3(nb), dim3(256), 0, h->stream, d.k1, n, d.file_off, (int)Fi, flags));
    tb = h->prim_tmp.cap;
    HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, tb, flags, pos, N, h->stream));
    LAUNCH(h, "mc_starts", hipLaunchKernelGGL(lk_pre_starts_kernel, dim3(nb), dim3(256), 0, h->stream, flags, pos, (int)n, d.starts, ncells_d));
    LAUNCH(h, "mc_celloff", hipLaunchKernelGGL(lk_dscan_celloff_kernel, dim3((Fi + 1 + 255) / 256), dim3(256), 0, h->stream, d.file_off, pos, ncells_d, (int)Fi,
                                               d.cell_off));
    // 3. the records into cell order, one centroid per cell
    LAUNCH(h, "mc_gather", hipLaunchKernelGGL(lk_mc_gather_kernel, dim3(nb), dim3(256), 0, h->stream, pts, d.v1, n, d.sorted));
    LAUNCH(h, "mc_centroid", hipLaunchKernelGGL(lk_mc_centroid_kernel, dim3(nb), dim3(256), 0, h->stream, d.sorted, d.starts, ncells_d, n, d.file_off, (int)Fi,
                                                d.grid, reinterpret_cast<float4*>(d_out)));
    std::vector<unsigned int> co(F + 1);
    HIPCHK(h, hipMemcpyAsync(co.data(), d.cell_off, 4 * (F + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t f = 0; f <= F; ++f) out_off[f] = co[f];
    if (unfiltered)
        for (size_t f = 0; f < F; ++f) unfiltered[f] = grid[LK_MC_GRID_WORDS * f + 6] ? 1 : 0;
    return LK_OK;
}

int lk_downsample_clouds(lk_handle* h, const float* world, size_t n_files, const uint64_t* file_off, float leaf, float* out, uint64_t* out_off,
                         uint8_t* unfiltered) {
    CHECK_H(h);
    size_t N = 0;
    LKCHK(mcl_check_tables(h, "lk_downsample_clouds", world, n_files, file_off, leaf, out, out_off, &N));
    MclPool d;
    LKCHK(mcl_reserve(h, N, n_files, N, d));
    HIPCHK(h, hipMemcpyAsync(d.io_in, world + 4 * file_off[0], 16 * N, hipMemcpyHostToDevice, h->stream));
    std::vector<uint64_t> rel(n_files + 1);
    for (size_t f = 0; f <= n_files; ++f) rel[f] = file_off[f] - file_off[0];
    LKCHK(lk_downsample_clouds_dev(h, reinterpret_cast<const float*>(d.io_in), n_files, rel.data(), leaf, reinterpret_cast<float*>(d.io_out), out_off,
                                   unfiltered));
    HIPCHK(h, hipMemcpyAsync(out, d.io_out, 16 * (size_t)out_off[n_files], hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

int lk_preprocess_scan(lk_handle* h, const lk_point* raw, size_t n_raw, float leaf, lk_point* out_sorted, size_t* n_out) {
    CHECK_H(h);
    if (!raw || !out_sorted || n_raw == 0) return fail(h, LK_ERR_INVALID, "lk_preprocess_scan: bad argument");
    FrontPool d;
    LKCHK(front_reserve(h, n_raw, 1, n_raw, sizeof(lk_point) * n_raw, d));
    HIPCHK(h, hipMemcpyAsync(d.io_in, raw, sizeof(lk_point) * n_raw, hipMemcpyHostToDevice, h->stream));
    LKCHK(lk_preprocess_scan_dev(h, reinterpret_cast<const lk_point*>(d.io_in), n_raw, leaf, d.io_out, n_out));
    HIPCHK(h, hipMemcpyAsync(out_sorted, d.io_out, sizeof(lk_point) * (*n_out), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

int lk_process_raw_scan(lk_handle* h, const lk_point* raw, size_t n_raw, float leaf, double t_begin, const lk_imu* imus,
                        size_t n_imu, const lk_kin_imu* kins, size_t n_kin, size_t* n_down, lk_pose* out) {
    CHECK_H(h);
    if (!raw || n_raw == 0) return fail(h, LK_ERR_INVALID, "empty scan");
    if (n_imu && n_kin) return fail(h, LK_ERR_INVALID, "pass either IMU or kin+IMU messages, not both");
    FrontPool d;
    LKCHK(front_reserve(h, n_raw, 1, n_raw, sizeof(lk_point) * n_raw, d));
    HIPCHK(h, hipMemcpyAsync(d.io_in, raw, sizeof(lk_point) * n_raw, hipMemcpyHostToDevice, h->stream));
    size_t nd = 0;
    LKCHK(lk_preprocess_scan_dev(h, reinterpret_cast<const lk_point*>(d.io_in), n_raw, leaf, d.io_out, &nd));
    if (nd > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "downsampled scan exceeds max_scan_points");
    std::vector<lk_point> sorted(nd);
    HIPCHK(h, hipMemcpyAsync(sorted.data(), d.io_out, sizeof(lk_point) * nd, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_down) *n_down = nd;
    return run_scan(h, sorted.data(), d.io_out, nd, t_begin, imus, n_imu, kins, n_kin, nullptr, out);
}

// ------------------------------------------------------------------ batch replay against the frozen map
int lk_batch_set_priors(lk_handle* h, const double* x36, const double* P900, size_t n_scans) {
    CHECK_H(h);
    if (n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans exceeds n_slots");
    HIPCHK(h, hipMemcpy2DAsync(h->d_filters[0].x, sizeof(LkFilter), x36, sizeof(double) * 36, sizeof(double) * 36, n_scans,
                               hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(h->d_filters[0].P, sizeof(LkFilter), P900, sizeof(double) * 900, sizeof(double) * 900, n_scans,
                               hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

int lk_batch_set_priors_dev(lk_handle* h, const double* d_x36, const double* d_P900, size_t n_scans) {
    CHECK_H(h);
    if (n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans exceeds n_slots");
    if (!d_x36 || !d_P900) return fail(h, LK_ERR_INVALID, "null prior buffer");
    HIPCHK(h, hipMemcpy2DAsync(h->d_filters[0].x, sizeof(LkFilter), d_x36, sizeof(double) * 36, sizeof(double) * 36, n_scans,
                               hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(h->d_filters[0].P, sizeof(LkFilter), d_P900, sizeof(double) * 900, sizeof(double) * 900, n_scans,
                               hipMemcpyDeviceToDevice, h->stream));
    return LK_OK;
}

// ---- a batch put into root-voxel order, bucket by bucket (lk_batch_sort_by_voxel_dev)
// key of point i of scan s: its root voxel under the slot's PRIOR pose (load_bucket_const / point_world / key_floor: what the first
// bucket's residual pass will compute), ten bits per axis - a wrap-around beyond 1 024 voxels only costs locality; value: the point's
// index in the batch
__global__ void __launch_bounds__(256)
    lk_sort_keys_kernel(LkParams pr, const LkFilter* __restrict__ filters, const lk_point* __restrict__ pts, size_t n_pts, unsigned int* __restrict__ keys,
                        unsigned int* __restrict__ vals) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pts) return;
    BucketConst bc;
    load_bucket_const<false>(&filters[blockIdx.y], pr, bc);
    const size_t j = (size_t)blockIdx.y * n_pts + i;
    const float4 p = reinterpret_cast<const float4*>(pts)[j];
    const V3 pw = point_world(p.x, p.y, p.z, bc, pr);
    int key[3];
    key_floor(pw, pr.voxel_size_f, key);
    keys[j] = (((unsigned int)key[2] & 1023u) << 20) | (((unsigned int)key[1] & 1023u) << 10) | ((unsigned int)key[0] & 1023u);
    vals[j] = (unsigned int)j;
}
__global__ void __launch_bounds__(256) lk_sort_gather_kernel(const lk_point* __restrict__ in, lk_point* __restrict__ out, const unsigned int* __restrict__ vals, size_t n) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) reinterpret_cast<float4*>(out)[j] = reinterpret_cast<const float4*>(in)[vals[j]];
}
// Every time bucket of every scan of a device-resident batch in root-voxel order: a residual wave's 64 points then look at a handful of voxels
// instead of sixty (1.8 -> 0.6 L2 requests per point on the bench batch, 2.25 -> 1.6 ms per step).  Points keep their bucket; the order inside
// a bucket is one of the legal outcomes of KILO.cc:369's sort (equal curvature).  Stable segmented radix sort (rocPRIM) of (key, index) pairs +
// one gather; priors from lk_batch_set_priors(_dev).  Once per loaded batch, not per replay; in and out must not overlap.
static int sort_by_voxel(lk_handle* h, const lk_point* d_in, lk_point* d_out, uint32_t first_slot, size_t n_scans, size_t n_pts, const uint32_t* bucket_off, size_t n_buckets);
int lk_batch_sort_by_voxel_dev(lk_handle* h, const lk_point* d_in, lk_point* d_out, size_t n_scans, size_t n_pts, const uint32_t* bucket_off, size_t n_buckets) {
    CHECK_H(h);
    return sort_by_voxel(h, d_in, d_out, 0, n_scans, n_pts, bucket_off, n_buckets);
}
static int sort_by_voxel(lk_handle* h, const lk_point* d_in, lk_point* d_out, uint32_t first_slot, size_t n_scans, size_t n_pts, const uint32_t* bucket_off, size_t n_buckets) {
    if (!d_in || !d_out || !bucket_off) return fail(h, LK_ERR_INVALID, "null argument");
    if (n_scans == 0 || n_pts == 0 || n_buckets == 0) return fail(h, LK_ERR_INVALID, "empty batch");
    if ((size_t)first_slot + n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans exceeds n_slots");
    if (bucket_off[0] != 0 || bucket_off[n_buckets] != n_pts) return fail(h, LK_ERR_INVALID, "bucket_off must cover the scan: bucket_off[0] == 0, bucket_off[n_buckets] == n_pts");
    for (size_t b = 0; b < n_buckets; ++b)
        if (bucket_off[b + 1] < bucket_off[b]) return fail(h, LK_ERR_INVALID, "bucket_off must be non-decreasing");
    const size_t total = n_scans * n_pts;
    if (total >= (size_t)1 << 32) return fail(h, LK_ERR_INVALID, "batch exceeds 2^32 points");
    const size_t nseg = n_scans * n_buckets;
    std::vector<unsigned int> offs(nseg + 1);
    for (size_t s = 0; s < n_scans; ++s)
        for (size_t b = 0; b < n_buckets; ++b) offs[s * n_buckets + b] = (unsigned int)(s * n_pts + bucket_off[b]);
    offs[nseg] = (unsigned int)total;
    DevTemps tmp;
    unsigned int *k0 = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr, *d_off = nullptr;
    void* d_tmp = nullptr;
    HIPCHK(h, tmp.alloc(&k0, sizeof(unsigned int) * total));
    HIPCHK(h, tmp.alloc(&k1, sizeof(unsigned int) * total));
    HIPCHK(h, tmp.alloc(&v0, sizeof(unsigned int) * total));
    HIPCHK(h, tmp.alloc(&v1, sizeof(unsigned int) * total));
    HIPCHK(h, tmp.alloc(&d_off, sizeof(unsigned int) * (nseg + 1)));
    HIPCHK(h, hipMemcpyAsync(d_off, offs.data(), sizeof(unsigned int) * (nseg + 1), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(lk_sort_keys_kernel, dim3((unsigned int)((n_pts + 255) / 256), (unsigned int)n_scans), dim3(256), 0, h->stream, h->pr, h->d_filters + first_slot, d_in, n_pts, k0, v0);
    HIPCHK(h, hipGetLastError());
    size_t tmp_bytes = 0;
    HIPCHK(h, lk_prim_segmented_sort_pairs(nullptr, tmp_bytes, k0, k1, v0, v1, (unsigned int)total, (unsigned int)nseg, d_off, d_off + 1, 0, 30, h->stream));
    HIPCHK(h, tmp.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 16)));
    HIPCHK(h, lk_prim_segmented_sort_pairs(d_tmp, tmp_bytes, k0, k1, v0, v1, (unsigned int)total, (unsigned int)nseg, d_off, d_off + 1, 0, 30, h->stream));
    hipLaunchKernelGGL(lk_sort_gather_kernel, dim3((unsigned int)((total + 255) / 256)), dim3(256), 0, h->stream, d_in, d_out, v1, total);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));   // offs and the temporaries go out of scope
    return LK_OK;
}

// ------------------------------------------------------------------ input order of device-resident batches (lk_batch_order)
// The batch residual kernel is 1.4 x slower on a batch whose buckets come in a random order than on one in voxel order (1.80 against 0.63 L2
// requests per point).  So that this is not the caller's problem, the frozen-map batch entries keep track of the batches they are given - (device
// pointer, shape, bucket bounds) + a stamp of 4 096 sampled points, taken ON THE DEVICE by a one-workgroup kernel ahead of the residual launches
// (no host round trip) - and once a batch has come back unchanged twice they sort it, unless every bucket already is in voxel order, ONCE into a
// library-owned copy (sort_by_voxel: 5.6 ms per 1 024 x 100 000 points) which its later replays read.  Any order inside a bucket is a legal outcome
// of the reference's sort of equal time stamps (KILO.cc:369), so the copy is a batch of the same scans.  A batch that is replayed once or twice - new
// scans streamed through one staging buffer - is never sorted; new content in a sorted batch's buffer is noticed by the same kernel, which tells the
// residual kernel to read the caller's buffer (ResidualOut::alt_use) and starts the count again.  (An in-place edit that changes none of the sampled
// points is not noticed: lk_batch_changed.)  The host picks the kernel's mode from a count that lags behind the replays in flight, so the device side
// is safe under ANY order of modes and stamps: the copy is read only by a replay that carries the stamp the copy was made from, which has a word of its
// own, and every ring stream of the asynchronous entry has its own decision word (lk_batch_stamp.h; tests/test_batch_stamp.py enumerates the orders).
__global__ void __launch_bounds__(256) lk_sort_check_kernel(LkParams pr, const LkFilter* __restrict__ filters, const lk_point* __restrict__ pts, size_t n_pts,
                                                            unsigned int* __restrict__ unsorted) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 || i >= n_pts) return;
    BucketConst bc;
    load_bucket_const<false>(&filters[blockIdx.y], pr, bc);
    const float4* p4 = reinterpret_cast<const float4*>(pts) + (size_t)blockIdx.y * n_pts;
    const float4 a = p4[i - 1], b = p4[i];
    if (a.w != b.w) return;   // a bucket boundary (runs of equal curvature, KILO.cc:375-378)
    int ka[3], kb[3];
    key_floor(point_world(a.x, a.y, a.z, bc, pr), pr.voxel_size_f, ka);
    key_floor(point_world(b.x, b.y, b.z, bc, pr), pr.voxel_size_f, kb);
    const unsigned int sa = (((unsigned int)ka[2] & 1023u) << 20) | (((unsigned int)ka[1] & 1023u) << 10) | ((unsigned int)ka[0] & 1023u);
    const unsigned int sb = (((unsigned int)kb[2] & 1023u) << 20) | (((unsigned int)kb[1] & 1023u) << 10) | ((unsigned int)kb[0] & 1023u);
    if (sb < sa) atomicAdd(unsorted, 1u);
}
// Stamp of 4 096 points spread over the batch, taken ahead of a replay's residual launches on the replay's own stream, and the replay's decision
// (lk_batch_stamp.h: lk_stamp_decide).  w: the batch's words - w[LK_ORDW_COPY] the stamp its copy was made from, written by LK_ORD_SET alone, apart
// from w[LK_ORDW_LAST], the stamp of the replay before, which only counts repeats.  use: the pair of the ring stream this replay runs on; use[1] = which
// buffer THIS replay's residual launches read (1: the library's copy, only if this replay's stamp is the copy's own) - a word per stream, so that no
// other stream's stamp kernel rewrites it under them.  *seen (host-mapped, atomic) = how many replays in a row have found the same stamp
// (LK_ORD_SORTED while a copy of this very content exists).
__global__ void __launch_bounds__(256) lk_batch_stamp_kernel(const lk_point* __restrict__ pts, size_t total, unsigned long long* __restrict__ w,
                                                             unsigned long long* __restrict__ use, unsigned int* __restrict__ seen, int mode) {
    __shared__ unsigned long long acc;
    if (threadIdx.x == 0) acc = 0ull;
    __syncthreads();
    const size_t stride = lk_stamp_stride(total);
    unsigned long long hsh = 0ull;
    for (int k = 0; k < LK_STAMP_SAMPLES / 256; ++k) {
        const size_t idx = ((size_t)threadIdx.x * (LK_STAMP_SAMPLES / 256) + k) * stride;
        if (idx >= total) break;
        const uint4 v = reinterpret_cast<const uint4*>(pts)[idx];
        hsh += lk_stamp_mix(v.x, v.y, v.z, v.w, idx);
    }
    atomicAdd(&acc, hsh);
    __syncthreads();
    if (threadIdx.x == 0) lk_stamp_decide(mode, lk_stamp_finish(acc), w, use, seen);
}
static uint64_t hash_offsets(const uint32_t* off, size_t n) {
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i <= n; ++i) x = (x ^ off[i]) * 1099511628211ull;
    return x;
}
// Which buffer the residual launches of a frozen-map batch replay read.  `st`: the stream the slots' priors were armed on and the batch will run on;
// `ring`: which of the LK_ORD_RINGS decision pairs of the batch's words this replay owns - the asynchronous entry's ring stream.  The synchronous
// entry passes 0 and makes this call on h->stream BEFORE its slot groups fork: all groups of one call read one pair, written before any of them starts.
// Fills ro->alt_pts / alt_use (null: the caller's buffer as given).  One small launch per call; the call that makes the copy synchronises.
static int batch_ordered(lk_handle* h, const lk_point* d_pts, uint32_t first_slot, size_t n_scans, size_t n_pts, const uint32_t* bucket_off, size_t n_buckets,
                         hipStream_t st, uint32_t ring, ResidualOut* ro, bool now = false) {
    ResidualOut none;
    if (!ro) ro = &none;
    ro->alt_pts = nullptr, ro->alt_use = nullptr;
    if (h->batch_order_mode == 0 || n_scans * n_pts < LK_STAMP_SAMPLES || n_scans * n_pts >= ((size_t)1 << 32)) return LK_OK;
    const auto drain = [&]() -> int {   // replays in flight on any stream read and write the entries' words
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i)
            if (h->side[i]) HIPCHK(h, hipStreamSynchronize(h->side[i]));
        return LK_OK;
    };
    const uint64_t oh = hash_offsets(bucket_off, n_buckets);
    lk_handle::OrdEntry* e = nullptr;
    for (auto& c : h->ord)
        if (c.src == d_pts && c.n_scans == n_scans && c.n_pts == n_pts && c.n_buckets == n_buckets && c.off_hash == oh) e = &c;
    if (!e) {   // a batch not seen before (or forgotten): the least recently used entry goes; nothing is examined yet, only its stamp is taken
        e = h->ord[0].tick <= h->ord[1].tick ? &h->ord[0] : &h->ord[1];
        if (!e->d_ref) {
            HIPCHK(h, hipMalloc(&e->d_ref, LK_ORDW_COUNT * sizeof(unsigned long long)));
            HIPCHK(h, hipHostMalloc(&e->h_seen, sizeof(unsigned int), hipHostMallocMapped));
            HIPCHK(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&e->d_seen), e->h_seen, 0));
        } else {
            LKCHK(drain());   // replays of the entry's former batch may still be using its words
        }
        *reinterpret_cast<volatile unsigned int*>(e->h_seen) = 0u;
        HIPCHK(h, hipMemsetAsync(e->d_ref, 0, LK_ORDW_COUNT * sizeof(unsigned long long), st));
        e->src = d_pts, e->n_scans = n_scans, e->n_pts = n_pts, e->n_buckets = n_buckets, e->off_hash = oh;
        e->as_given = false, e->have_copy = false;
        e->probes = 0, e->waited = false;
    }
    e->tick = ++h->ord_tick;
    if (e->as_given) return LK_OK;
    const auto count = [&]() { return *reinterpret_cast<volatile unsigned int*>(e->h_seen); };   // written by the device; may lag behind the replays still in flight
    unsigned int seen = count();
    if (e->have_copy && seen < LK_ORD_SORTED) {   // a replay found other content in the caller's buffer: the copy is of no use any more
        e->have_copy = false;
        e->probes = 1, e->waited = false;         // (that replay was the new content's first)
        ++h->ord_stale;
    }
    if (!e->have_copy && !now && !e->waited && e->probes >= (unsigned int)h->batch_order_after && seen < (unsigned int)h->batch_order_after) {
        // enough replays are enqueued for the count to be there, but it is not (yet): this may be the replay that sorts.  Wait for the ones in flight,
        // once per content - the sort would wait for them anyway; a buffer whose content keeps changing pays this a single time
        LKCHK(drain());
        e->waited = true;
        seen = count();
    }
    unsigned long long* use = e->d_ref + LK_ORDW_USE + 2 * ring;
    if (!e->have_copy && (now || seen >= (unsigned int)h->batch_order_after) && seen < LK_ORD_SORTED) {
        // the same content has been replayed often enough to be worth 5.6 ms: examine it, and unless it already is in voxel order, sort it into the copy
        ++h->ord_examined;
        HIPCHK(h, hipStreamSynchronize(st));   // the priors are armed
        LKCHK(drain());
        unsigned int* d_uns = reinterpret_cast<unsigned int*>(e->d_ref + LK_ORDW_SCRATCH);
        HIPCHK(h, hipMemsetAsync(d_uns, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(lk_sort_check_kernel, dim3((unsigned int)((n_pts + 255) / 256), (unsigned int)n_scans), dim3(256), 0, st, h->pr, h->d_filters + first_slot, d_pts, n_pts, d_uns);
        HIPCHK(h, hipGetLastError());
        unsigned int uns = 0;
        HIPCHK(h, hipMemcpyAsync(&uns, d_uns, sizeof(uns), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        bool sort_it = uns != 0;
        if (sort_it) {
            const size_t bytes = sizeof(lk_point) * n_scans * n_pts;
            if (e->copy_bytes < bytes) {
                if (e->copy) hipFree(e->copy), e->copy = nullptr, e->copy_bytes = 0;
                if (hipMalloc(&e->copy, bytes) != hipSuccess) {   // no room for a copy: this batch is replayed as given
                    (void)hipGetLastError();
                    e->copy = nullptr;
                    sort_it = false;
                } else {
                    e->copy_bytes = bytes;
                }
            }
        }
        if (!sort_it) {
            e->as_given = true;   // in voxel order already (or no memory): replayed where it lies from now on, no stamps
            return LK_OK;
        }
        const int rc = sort_by_voxel(h, d_pts, e->copy, first_slot, n_scans, n_pts, bucket_off, n_buckets);   // on h->stream, synchronous
        if (rc) return rc;
        ++h->ord_sorted;
        e->have_copy = true;
        hipLaunchKernelGGL(lk_batch_stamp_kernel, dim3(1), dim3(256), 0, st, d_pts, n_scans * n_pts, e->d_ref, use, e->d_seen, LK_ORD_SET);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(st));
    } else {
        hipLaunchKernelGGL(lk_batch_stamp_kernel, dim3(1), dim3(256), 0, st, d_pts, n_scans * n_pts, e->d_ref, use, e->d_seen, e->have_copy ? LK_ORD_CHECK : LK_ORD_PROBE);
        HIPCHK(h, hipGetLastError());
        if (!e->have_copy) ++e->probes;
    }
    if (e->have_copy) ro->alt_pts = e->copy, ro->alt_use = use;
    return LK_OK;
}

// one workgroup per slot: state and covariance of a filter slot into dense [n][36] / [n][900] arrays
__global__ void __launch_bounds__(256) lk_states_gather_kernel(const LkFilter* __restrict__ filters, double* __restrict__ x36, double* __restrict__ P900) {
    const LkFilter* f = &filters[blockIdx.x];
    if (x36 && threadIdx.x < LK_STATE_DOUBLES) x36[(size_t)blockIdx.x * LK_STATE_DOUBLES + threadIdx.x] = f->x[threadIdx.x];
    if (P900)
        for (int e = threadIdx.x; e < 900; e += 256) P900[(size_t)blockIdx.x * 900 + e] = f->P[e];
}
int join_side_streams(lk_handle* h) {   // the asynchronous batch entry may still be running on a side stream
    for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i)
        if (h->side[i]) {
            HIPCHK(h, hipEventRecord(h->ev_join[i], h->side[i]));
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join[i], 0));
        }
    return LK_OK;
}
int lk_batch_order(lk_handle* h, int mode) {
    CHECK_H(h);
    if (mode != 0 && mode != 1) return fail(h, LK_ERR_INVALID, "mode must be LK_BATCH_ORDER_AS_GIVEN (0) or LK_BATCH_ORDER_AUTO (1)");
    h->batch_order_mode = mode;
    return LK_OK;
}
int lk_batch_prepare_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, const uint32_t* bucket_off, size_t n_buckets) {
    CHECK_H(h);
    if (!d_pts || !bucket_off) return fail(h, LK_ERR_INVALID, "null argument");
    if (n_scans == 0 || n_scans > h->cfg.n_slots || n_pts == 0 || n_buckets == 0) return fail(h, LK_ERR_INVALID, "empty batch, or n_scans exceeds n_slots");
    if (bucket_off[0] != 0 || bucket_off[n_buckets] != n_pts) return fail(h, LK_ERR_INVALID, "bucket_off must cover the scan: bucket_off[0] == 0, bucket_off[n_buckets] == n_pts");
    if (h->batch_order_mode == 0) return LK_OK;   // LK_BATCH_ORDER_AS_GIVEN: no replay would read the copy
    int rc = join_side_streams(h);
    if (rc) return rc;
    rc = batch_ordered(h, d_pts, 0, n_scans, n_pts, bucket_off, n_buckets, h->stream, 0, nullptr, true);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_batch_changed(lk_handle* h) {
    CHECK_H(h);
    for (auto& e : h->ord) e.src = nullptr;   // every batch is a first sight again (the copies' memory is kept for the next one)
    return LK_OK;
}
int lk_batch_order_stats(lk_handle* h, uint64_t* out3) {
    CHECK_H(h);
    if (!out3) return fail(h, LK_ERR_INVALID, "null argument");
    out3[0] = h->ord_examined, out3[1] = h->ord_sorted, out3[2] = h->ord_stale;
    return LK_OK;
}
int lk_batch_get_states_dev(lk_handle* h, uint32_t first_slot, size_t n, double* d_x36, double* d_P900) {
    CHECK_H(h);
    if (n == 0) return LK_OK;
    if ((size_t)first_slot + n > (size_t)h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "slot range exceeds n_slots");
    int rc = join_side_streams(h);
    if (rc) return rc;
    hipLaunchKernelGGL(lk_states_gather_kernel, dim3((unsigned int)n), dim3(256), 0, h->stream, h->d_filters + first_slot, d_x36, d_P900);
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}
int lk_batch_get_states(lk_handle* h, uint32_t first_slot, size_t n, double* x36, double* P900) {
    CHECK_H(h);
    if (n == 0) return LK_OK;
    if ((size_t)first_slot + n > (size_t)h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "slot range exceeds n_slots");
    DevTemps tmp;
    double *d_x = nullptr, *d_P = nullptr;
    if (x36) HIPCHK(h, tmp.alloc(&d_x, sizeof(double) * LK_STATE_DOUBLES * n));
    if (P900) HIPCHK(h, tmp.alloc(&d_P, sizeof(double) * 900 * n));
    int rc = lk_batch_get_states_dev(h, first_slot, n, d_x, d_P);
    if (rc) return rc;
    if (x36) HIPCHK(h, hipMemcpyAsync(x36, d_x, sizeof(double) * LK_STATE_DOUBLES * n, hipMemcpyDeviceToHost, h->stream));
    if (P900) HIPCHK(h, hipMemcpyAsync(P900, d_P, sizeof(double) * 900 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

__global__ void lk_set_times_kernel(LkFilter* filters, int n, double t) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) filters[s].last_predict_t = t, filters[s].last_update_t = t;
}

// The frozen-map bucket chain of `sn` slots from filter slot `s0` on, all of it on stream `st`: predict -> (residual -> update + next predict) per
// live bucket - update(k) and predict(k+1) share one launch (the map is frozen: nothing reads the state in between).  pts / alt_pts: the first
// point of slot s0 in the caller's buffer and in the library's voxel-ordered copy (null: none); ro: what batch_ordered filled in.
// named: through launch() as "predict" / "residual" / "update" (what lk_profile_get hands back: the one-stream synchronous path); else plain
// launches, checked once at the end.
static int enqueue_frozen_chain(lk_handle* h, hipStream_t st, bool named, uint32_t s0, int sn, const lk_point* pts, const lk_point* alt_pts, size_t n_pts,
                                const std::vector<size_t>& live, const uint32_t* bucket_off, const double* bucket_dt, double t_begin, const LkMap& fmap,
                                ResidualOut ro) {
    const auto go = [&](const char* name, auto&& f) -> int {
        if (named) return launch(h, name, f);
        f();
        return LK_OK;
    };
    const auto res_kernel = batch_residual_kernel(h, fmap);
    const bool wave = h->wave_update;   // the single-wave update kernel, or the 256-thread pair (LEGKILO_UPDATE_CLASSIC=1)
    LkFilter* fl = h->d_filters + s0;
    double* parts = h->d_partials + (size_t)s0 * h->part_stride;
    // the update at time t over n_tiles partial sums and / or the predict to t_next.  Last argument - wave kernel: 1 update, 2 predict, 3 both;
    // classic update kernel: 1 = predict after the update
    const auto update = [&](int n_tiles, double t, double t_next, bool upd, bool pred) {
        if (wave)
            hipLaunchKernelGGL(lk_update_wave_kernel, dim3(sn), dim3(LK_WAVE), 0, st, fl, parts, n_tiles, h->part_stride, t, h->d_Q, t_next, (upd ? 1 : 0) | (pred ? 2 : 0));
        else if (upd)
            hipLaunchKernelGGL(lk_update_kernel, dim3(sn), dim3(LK_FB), 0, st, fl, parts, n_tiles, h->part_stride, t, h->d_Q, t_next, pred ? 1 : 0);
        else
            hipLaunchKernelGGL(lk_predict_kernel, dim3(sn), dim3(LK_FB), 0, st, fl, h->d_Q, t_next);
    };
    for (size_t k = 0; k < live.size(); ++k) {
        const size_t b = live[k];
        const int nb = (int)(bucket_off[b + 1] - bucket_off[b]);
        const double t = t_begin + bucket_dt[b];
        const bool has_next = k + 1 < live.size();
        const double t_next = has_next ? t_begin + bucket_dt[live[k + 1]] : 0.0;
        const int nblk = (nb + LK_RB - 1) / LK_RB;
        if (k == 0) LKCHK(go("predict", [&]() { update(0, 0.0, t, false, true); }));
        ro.alt_pts = alt_pts ? alt_pts + bucket_off[b] : nullptr;
        const dim3 rgrid = batch_residual_grid(nblk, sn, &ro);
        LKCHK(go("residual", [&]() { hipLaunchKernelGGL(res_kernel, rgrid, dim3(LK_RB), 0, st, fmap, h->pr, fl, pts + bucket_off[b], n_pts, nb, parts, h->part_stride, ro, (size_t)0); }));
        LKCHK(go("update", [&]() { update(nblk * (LK_RB / LK_WAVE), t, t_next, true, has_next); }));
    }
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}

int lk_batch_replay_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, double t_begin,
                        const uint32_t* bucket_off, const double* bucket_dt, size_t n_buckets, lk_pose* out) {
    CHECK_H(h);
    if (n_scans == 0 || n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans must be in [1, n_slots]");
    if (n_pts == 0 || n_buckets == 0) return fail(h, LK_ERR_INVALID, "empty scans");
    const int S = (int)n_scans;
    std::vector<size_t> live;
    LKCHK(live_buckets(h, bucket_off, n_buckets, live));   // all checks before the first enqueue
    LkMap fmap;
    LKCHK(frozen_map(h, &fmap));
    h->bucket_n = 0;   // (a batch replay that records no buckets: lk_runs_bucket_poses)
    LKCHK(zero_scan_counters(h, 0, (uint32_t)n_scans));
    hipLaunchKernelGGL(lk_set_times_kernel, dim3((S + 63) / 64), dim3(64), 0, h->stream, h->d_filters, S, t_begin);
    HIPCHK(h, hipGetLastError());
    ResidualOut ro;
    memset(&ro, 0, sizeof(ro));
    LKCHK(batch_ordered(h, d_pts, 0, n_scans, n_pts, bucket_off, n_buckets, h->stream, 0, &ro));   // the caller's buffer, or the library's voxel-ordered copy of it: decided on h->stream, before the groups fork
    // the single-workgroup update / predict kernels of one group (half of the CUs idle, latency-bound) overlap the residual kernel of the other group
    const SlotGroups grp(h, S, h->replay_groups, kReplayGroupSlots);
    LKCHK(grp.fork());
    int rc = LK_OK;
    for (int g = 0; g < grp.n && rc == LK_OK; ++g) {
        const size_t p0 = (size_t)grp.first(g) * n_pts;
        rc = enqueue_frozen_chain(h, grp.stream[g], grp.n == 1, (uint32_t)grp.first(g), grp.count(g), d_pts + p0, ro.alt_pts ? ro.alt_pts + p0 : nullptr, n_pts, live,
                                  bucket_off, bucket_dt, t_begin, fmap, ro);
    }
    LKCHK(grp.join(rc));
    return fetch_poses_or_sync(h, out, S);
}

// Config 2 at bandwidth size: the residual build of KILO.cc:122-210 - transform, covariance terms, voxel lookup, plane match with the one
// neighbour retry, observation row - for n_scans x n_pts points in ONE launch, scan s under the CURRENT state of filter slot s (no predict,
// no update, no insert), rows MATERIALISED in HBM: one 64-B record [h(6) z R] per point + the valid byte lk_residuals returns.
// 16 B in + 65 B out per point; the map side is the frozen-map grid of the batch replay (L2 / Infinity-Cache resident).
int lk_batch_residuals_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, double* d_rows8, uint8_t* d_valid) {
    CHECK_H(h);
    if (!d_pts || !d_rows8 || !d_valid) return fail(h, LK_ERR_INVALID, "null argument");
    if (((uintptr_t)d_rows8 & 15u) != 0) return fail(h, LK_ERR_INVALID, "d_rows8 must be 16-byte aligned");
    if (n_scans == 0 || n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans must be in [1, n_slots]");
    if (n_pts == 0) return fail(h, LK_ERR_INVALID, "empty scans");
    if (n_pts > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "n_pts exceeds max_scan_points");
    LkMap fmap;
    int rc = frozen_map(h, &fmap);
    if (rc) return rc;
    rc = join_side_streams(h);
    if (rc) return rc;
    const ResidualKernelFn k = !fmap.grid_on ? lk_residual_kernel<true, 0, false>
                                             : ((h->pr.ext_identity && lk_xid_enabled()) ? lk_residual_kernel<true, 1, true> : lk_residual_kernel<true, 1, false>);
    ResidualOut ro;
    memset(&ro, 0, sizeof(ro));
    ro.rows8 = d_rows8, ro.valid = d_valid;
    const int nblk = (int)((n_pts + LK_RB - 1) / LK_RB);
    const dim3 rgrid = batch_residual_grid(nblk, (int)n_scans, &ro);
    LAUNCH(h, "residual_rows", hipLaunchKernelGGL(k, rgrid, dim3(LK_RB), 0, h->stream, fmap, h->pr, h->d_filters, d_pts, n_pts, (int)n_pts,
                                                  h->d_partials, h->part_stride, ro, n_pts));
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}

#ifdef LK_DEBUG_PROLOGUE
// DEBUG BUILD ONLY: the batch residual kernel's phase clocks (lk_res_phase_dbg, lk_point_kernels.h) of this translation unit's launches - the
// frozen-map batch entries - since the last call, in ticks of 10 ns; reset behind the read.  Not declared in include/legkilo_hip.h.
extern "C" int lk_debug_res_phases(unsigned long long* out8) {
    if (hipDeviceSynchronize() != hipSuccess) return LK_ERR_HIP;
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(lk_res_phase_dbg), 8 * sizeof(unsigned long long)) != hipSuccess) return LK_ERR_HIP;
    const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(lk_res_phase_dbg), zero, sizeof(zero)) == hipSuccess ? LK_OK : LK_ERR_HIP;
}
#endif
#ifdef LK_DEBUG_PHASES
// the one-wave-per-scan kernels' phase clocks (lk_sw_dbg), printed and reset
static void dump_scan_wave_phases(hipStream_t st) {
    unsigned long long hb[16];
    hipStreamSynchronize(st);
    hipMemcpyFromSymbol(hb, HIP_SYMBOL(lk_sw_dbg), sizeof(hb));
    const char* names[6] = {"head", "predict", "bc", "residual", "update", "tail"};
    fprintf(stderr, "[scan-wave phases] %llu buckets:", hb[15]);
    for (int k = 0; k < 6; ++k) fprintf(stderr, " %s %.2f us;", names[k], (double)hb[k] / (double)hb[15] * 0.01);
    fprintf(stderr, "\n");
    memset(hb, 0, sizeof(hb));
    hipMemcpyToSymbol(HIP_SYMBOL(lk_sw_dbg), hb, sizeof(hb));
}
#endif
// The launches of a ragged batch once its tables (padded or CSR, LkRagged) are in HBM.  msg_kind: a MsgKind.
// max_n: largest bucket of every bucket index (null: `biggest` for all of them).  d_tbegin: the slots' start times, or null - they go on from the
// time stamps they hold (LK_RUNS_CONTINUE).  Runs (rg.run_scan, CSR tables: lk_batch_replay_runs_dev): a slot is a run of scans - for addressing and
// time one long scan of ldb buckets at most; the kernels know where its scans end, and `out` takes the n_poses records of rg.scan_pose instead of
// the slots' poses.
static int ragged_launch(lk_handle* h, const lk_point* d_pts, size_t S, const LkRagged& rg, const double* d_tbegin, int biggest, size_t ldb,
                         const int* max_n, int msg_kind, lk_pose* out, size_t n_poses = 0) {
    LkMap fmap;
    int rc = frozen_map(h, &fmap);
    if (rc) return rc;
    h->bucket_n = 0;   // (the _cloud entry sets it behind its replay)
    rc = zero_scan_counters(h, 0, (uint32_t)S);
    if (rc) return rc;
    hipStream_t st = h->stream;
    LkFilter* fl = h->d_filters;
    const bool runs = rg.run_scan != nullptr;
    if (d_tbegin) hipLaunchKernelGGL(lk_set_times_ragged_kernel, dim3(((int)S + 63) / 64), dim3(64), 0, st, fl, (int)S, d_tbegin);
    if (biggest <= LK_SCAN_WAVE_MAX && (msg_kind || !getenv("LEGKILO_RAGGED_LEVELS"))) {
        // small buckets only (a real scan's 2 ms bins): each scan's (run's) whole bucket chain as one wave, one launch
        if (runs) {
            const auto run_kernel = msg_kind == MSG_KIN ? lk_run_wave_kin_kernel : msg_kind == MSG_IMU ? lk_run_wave_imu_kernel : lk_run_wave_kernel;
            hipLaunchKernelGGL(run_kernel, dim3((unsigned)S), dim3(LK_WAVE), 0, st, fmap, h->pr, fl, d_pts, rg, h->d_Q);
        } else if (msg_kind == MSG_KIN)
            hipLaunchKernelGGL(lk_scan_wave_kin_kernel, dim3((unsigned)S), dim3(LK_WAVE), 0, st, fmap, h->pr, fl, d_pts, rg, h->d_Q);
        else if (msg_kind == MSG_IMU)
            hipLaunchKernelGGL(lk_scan_wave_imu_kernel, dim3((unsigned)S), dim3(LK_WAVE), 0, st, fmap, h->pr, fl, d_pts, rg, h->d_Q);
        else
            hipLaunchKernelGGL(lk_scan_wave_kernel, dim3((unsigned)S), dim3(LK_WAVE), 0, st, fmap, h->pr, fl, d_pts, rg, h->d_Q);
#ifdef LK_DEBUG_PHASES
        dump_scan_wave_phases(st);
#endif
        ldb = 0;
    } else {
        hipLaunchKernelGGL(lk_update_wave_ragged_kernel, dim3((unsigned)S), dim3(LK_WAVE), 0, st, fl, h->d_partials, h->part_stride, h->d_Q, rg, -1);
    }
    for (size_t b = 0; b < ldb; ++b) {
        const int nblk = ((max_n ? max_n[b] : biggest) + LK_RB - 1) / LK_RB;
        const auto rag_kernel = fmap.grid_on ? lk_residual_ragged_kernel<1> : lk_residual_ragged_kernel<0>;
        hipLaunchKernelGGL(rag_kernel, dim3(nblk, (unsigned)S), dim3(LK_RB), 0, st, fmap, h->pr, fl, d_pts, rg, (int)b, h->d_partials,
                           h->part_stride);
        // runs: the update alone, then the pose tap and the predict to the next bucket (lk_run_tap_predict_kernel) - the same arithmetic in two launches
        hipLaunchKernelGGL(lk_update_wave_ragged_kernel, dim3((unsigned)S), dim3(LK_WAVE), 0, st, fl, h->d_partials, h->part_stride, h->d_Q, rg,
                           (int)b, runs ? 1 : 0);
        if (runs) hipLaunchKernelGGL(lk_run_tap_predict_kernel, dim3((unsigned)S), dim3(LK_WAVE), 0, st, fl, h->d_Q, rg, (int)b);
    }
    HIPCHK(h, hipGetLastError());
    if (runs && out) {   // the scans' poses, written where each scan ended
        HIPCHK(h, hipMemcpyAsync(out, rg.scan_pose, sizeof(lk_pose) * n_poses, hipMemcpyDeviceToHost, st));
        out = nullptr;
    }
    return fetch_poses_or_sync(h, out, (int)S);
}

// Ragged batch replay: the scans of a recorded run differ in size, in their time buckets and in their start time.  One
// launch per bucket INDEX over all scans (grid sized by the largest bucket of that index; scans that have run out of
// buckets leave at once), every scan reading its own tables (LkRagged).  Same kernels' arithmetic as the uniform entry:
// a ragged batch of equally shaped scans gives the same bits.  Synchronous; priors as for lk_batch_replay_dev.
int ragged_replay(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off,
                         const uint32_t* n_buckets, const uint32_t* bucket_off, const double* bucket_dt,
                         const double* t_begin, const uint32_t* n_imu, const void* imus, int msg_kind, lk_pose* out, bool with_insert) {
    CHECK_H(h);
    if (n_scans == 0 || n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans must be in [1, n_slots]");
    if (!d_pts || !scan_off || !n_buckets || !bucket_off || !bucket_dt || !t_begin) return fail(h, LK_ERR_INVALID, "null argument");
    const size_t S = n_scans;
    // pass 1: validate, count the non-empty buckets of every scan (empty ones are skipped, as in the uniform entry), pitch
    std::vector<uint32_t> cnt(S);
    size_t row_o = 0, row_t = 0, ldb = 0;
    uint32_t biggest_bucket = 0;
    for (size_t s = 0; s < S; ++s) {
        const uint32_t* bo = bucket_off + row_o;
        const size_t nbs = n_buckets[s];
        if (nbs == 0) return fail(h, LK_ERR_INVALID, "a scan has no buckets");
        if (bo[0] != 0 || scan_off[s] + bo[nbs] != scan_off[s + 1]) return fail(h, LK_ERR_INVALID, "bucket offsets do not tile the scan");
        uint32_t c = 0;
        const double* bt = bucket_dt + row_t;
        for (size_t b = 0; b < nbs; ++b) {
            // the same ordering rule the device-built tables enforce (lk_rag_flag_kernel): time stamps finite and non-decreasing
            if (!std::isfinite(bt[b]) || (b > 0 && bt[b] < bt[b - 1])) return fail(h, LK_ERR_INVALID, "bucket times must be finite and non-decreasing (KILO.cc:367-370 sorts the scan by time)");
            if (bo[b + 1] < bo[b]) return fail(h, LK_ERR_INVALID, "bucket offsets must be non-decreasing");
            if ((size_t)(bo[b + 1] - bo[b]) > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "bucket exceeds max_scan_points");
            c += bo[b + 1] > bo[b];
            biggest_bucket = std::max(biggest_bucket, bo[b + 1] - bo[b]);
        }
        if (c == 0) return fail(h, LK_ERR_INVALID, "empty scan");
        cnt[s] = c;
        ldb = std::max(ldb, (size_t)c);
        row_o += nbs + 1, row_t += nbs;
    }
    // every check comes before the first memset / upload / launch: a refused call leaves the filter slots untouched
    if (n_imu && biggest_bucket > (uint32_t)LK_SCAN_WAVE_MAX && !with_insert)   // (the batch with insert runs bucket by bucket: lk_rag_advance_kernel takes the messages at any bucket size)
        return fail(h, LK_ERR_INVALID, "IMU / kinematic messages between buckets are only replayed for scans whose buckets hold <= 512 points");
    size_t n_imu_total = 0;
    if (n_imu)
        for (size_t s = 0; s < S; ++s) n_imu_total += n_imu[s];
    if (n_imu_total && !imus) return fail(h, LK_ERR_INVALID, "null message array");
    const size_t msg_bytes = msg_record_bytes(msg_kind);
    struct Tables {   // staged in pinned host memory, uploaded in one copy
        unsigned long long* po;   // [S][ldb+1]
        double *t, *tb;           // [S][ldb], [S]
        unsigned char* im;        // the messages
        unsigned int *nb, *io;    // [S], [S+1]
        size_t bytes;
    };
    auto tables = [&](void* base) {   // one description: counted, then laid over the staging copy and over the device copy
        LkCarve c(base);
        Tables r;
        r.po = c.take<unsigned long long>(S * (ldb + 1)), r.t = c.take<double>(S * ldb), r.tb = c.take<double>(S);
        r.im = c.take<unsigned char>(msg_bytes * n_imu_total);
        r.nb = c.take<unsigned int>(S), r.io = c.take<unsigned int>(S + 1);
        r.bytes = c.total();
        return r;
    };
    const size_t bytes = tables(nullptr).bytes;
    LKCHK(rag_reserve(h, bytes));   // (synchronises: the previous call's upload from the staging buffer has completed)
    const Tables hs = tables(h->rag_stage.p), dv = tables(h->rag.p);
    std::vector<int> max_n(ldb, 0);
    row_o = 0, row_t = 0;
    for (size_t s = 0; s < S; ++s) {   // pass 2: fill
        const uint32_t* bo = bucket_off + row_o;
        const double* bd = bucket_dt + row_t;
        const size_t nbs = n_buckets[s];
        unsigned long long* po = hs.po + s * (ldb + 1);
        double* tr = hs.t + s * ldb;
        size_t k = 0;
        for (size_t b = 0; b < nbs; ++b) {
            if (bo[b + 1] == bo[b]) continue;
            po[k] = scan_off[s] + bo[b];
            tr[k] = t_begin[s] + bd[b];
            max_n[k] = std::max(max_n[k], (int)(bo[b + 1] - bo[b]));
            ++k;
        }
        for (size_t b = k; b <= ldb; ++b) po[b] = scan_off[s + 1];
        for (size_t b = k; b < ldb; ++b) tr[b] = 0.0;
        hs.tb[s] = t_begin[s];
        hs.nb[s] = cnt[s];
        row_o += nbs + 1, row_t += nbs;
    }
    if (n_imu) {
        if (n_imu_total) memcpy(hs.im, imus, msg_bytes * n_imu_total);
        hs.io[0] = 0;
        for (size_t s = 0; s < S; ++s) hs.io[s + 1] = hs.io[s] + n_imu[s];
    }
    HIPCHK(h, hipMemcpyAsync(h->rag.p, h->rag_stage.p, bytes, hipMemcpyHostToDevice, h->stream));
    LkRagged rg;
    rg.pt_off = dv.po;
    rg.t = dv.t;
    rg.nb = dv.nb;
    rg.ldb = (int)ldb;
    rg.imu_off = n_imu ? dv.io : nullptr;
    rg.imu = reinterpret_cast<const double*>(dv.im);
    rag_from_handle(h, msg_kind, &rg);
    rg.bstart = nullptr;
    if (with_insert) {
        size_t max_scan_pts = 0;
        for (size_t s = 0; s < S; ++s) max_scan_pts = std::max(max_scan_pts, (size_t)(scan_off[s + 1] - scan_off[s]));
        return overlay_ragged_launch(h, d_pts, S, rg, dv.tb, (int)biggest_bucket, ldb, max_n.data(), max_scan_pts, msg_kind, out);
    }
    return ragged_launch(h, d_pts, S, rg, dv.tb, (int)biggest_bucket, ldb, max_n.data(), msg_kind, out);
}

int lk_batch_replay_ragged_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off,
                               const uint32_t* n_buckets, const uint32_t* bucket_off, const double* bucket_dt,
                               const double* t_begin, lk_pose* out) {
    return ragged_replay(h, d_pts, n_scans, scan_off, n_buckets, bucket_off, bucket_dt, t_begin, nullptr, nullptr, MSG_NONE, out);
}
// The same with each scan's IMU messages (only_imu_use mode, KILO.cc:379-383): n_imu[s] messages of scan s, concatenated in
// `imus`, time-sorted per scan; a message stamped before a bucket's time is applied before that bucket, the rest of the
// scan's messages are left unused exactly as the bucket loop of KILO::process leaves them.
int lk_batch_replay_ragged_imu_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off,
                                   const uint32_t* n_buckets, const uint32_t* bucket_off, const double* bucket_dt,
                                   const double* t_begin, const uint32_t* n_imu, const lk_imu* imus, lk_pose* out) {
    CHECK_H(h);
    if (!n_imu) return fail(h, LK_ERR_INVALID, "null argument");
    return ragged_replay(h, d_pts, n_scans, scan_off, n_buckets, bucket_off, bucket_dt, t_begin, n_imu, imus, MSG_IMU, out);
}
// Leg-fusion mode (only_imu_use: false, the reference's default): n_kin[s] kinematic + IMU messages of scan s, concatenated in
// `kins`, time-sorted per scan; a message stamped before a bucket's time is applied (predictUpdateKinImu, KILO.cc:260-314:
// two predicts, 6 IMU rows + 3 rows per foot in contact, updateByKinImu eskf.cc:137-145) before that bucket, as the loop at
// KILO.cc:384-390 does.  Same bucket-size limit as the IMU entry.
int lk_batch_replay_ragged_kin_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off,
                                   const uint32_t* n_buckets, const uint32_t* bucket_off, const double* bucket_dt,
                                   const double* t_begin, const uint32_t* n_kin, const lk_kin_imu* kins, lk_pose* out) {
    CHECK_H(h);
    if (!n_kin) return fail(h, LK_ERR_INVALID, "null argument");
    return ragged_replay(h, d_pts, n_scans, scan_off, n_buckets, bucket_off, bucket_dt, t_begin, n_kin, kins, MSG_KIN, out);
}

// Recorded-run replay WITHOUT host-side bucket tables: the scans lie back to back in HBM (scan s = d_pts[scan_off[s] .. scan_off[s+1]),
// time-sorted), and the runs of equal curvature that KILO::process turns into buckets (KILO.cc:375-378) are found on the device
// (lk_rag_flag / rocPRIM exclusive scan / lk_rag_scatter: CSR tables in HBM); the host sends S + 1 offsets and S start times and
// reads back three integers.  msgs: n_msg[s] lk_imu (msg_kind 1) or lk_kin_imu (msg_kind 2) records per scan, concatenated, or
// msg_kind 0.  Same kernels, same results as lk_batch_replay_ragged(_imu / _kin)_dev with host-built tables.
int lk_batch_replay_scans_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin,
                              int msg_kind, const uint32_t* n_msg, const void* msgs, lk_pose* out) {
    CHECK_H(h);
    return replay_scans(h, d_pts, n_scans, scan_off, t_begin, msg_kind, n_msg, msgs, false, out);
}
// The same with the kinematic records already in HBM (lk_decode_highstate_dev + lk_kin_split_dev): a device-to-device copy instead of the upload.
int lk_batch_replay_scans_kin_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin,
                                  const uint32_t* n_msg, const lk_kin_imu* d_kins, lk_pose* out) {
    CHECK_H(h);
    if (!n_msg) return fail(h, LK_ERR_INVALID, "null argument");
    return replay_scans(h, d_pts, n_scans, scan_off, t_begin, MSG_KIN, n_msg, d_kins, true, out);
}
// ... and the IMU records (lk_decode_imu_dev + lk_imu_split_dev).
int lk_batch_replay_scans_imu_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin,
                                  const uint32_t* n_msg, const lk_imu* d_imus, lk_pose* out) {
    CHECK_H(h);
    if (!n_msg) return fail(h, LK_ERR_INVALID, "null argument");
    return replay_scans(h, d_pts, n_scans, scan_off, t_begin, MSG_IMU, n_msg, d_imus, true, out);
}
// The CSR bucket tables of scans that lie back to back in HBM, built on the device (lk_rag_flag / rocPRIM exclusive scan / lk_rag_scatter): what the
// batch replay of a recorded run (replay_scans) and a live run (run_tables) share.  take() names the arrays once, in the caller's carve of
// h->ragdev - first over a null base to count, then over the buffer -; build() fills them, and the caller's own kernel reads the status words next.
struct BucketTables {
    unsigned long long *so, *ps;   // [S + 1] scan offsets from the first scan's first point; [n + 1] first point of every bucket
    double *t0, *tb;               // [S] start time of every scan; [n] time of every bucket
    unsigned int *fl, *rk;         // [n] bucket-start flags, their ranks
    unsigned int *bs, *mo;         // [S + 1] first bucket / first message of every scan
    unsigned int* st;              // [8] status words (lk_pre_kernels.h)
    std::vector<unsigned long long> h_so;   // what the uploads read: alive as long as the tables
    std::vector<unsigned int> h_mo;
    void take(LkCarve& c, size_t n, size_t S) {
        so = c.take<unsigned long long>(S + 1), t0 = c.take<double>(S);
        ps = c.take<unsigned long long>(n + 1), tb = c.take<double>(n);
        fl = c.take<unsigned int>(n), rk = c.take<unsigned int>(n);
        bs = c.take<unsigned int>(S + 1), mo = c.take<unsigned int>(S + 1);
        st = c.take<unsigned int>(8);
    }
    // d_pts: the first scan's first point (scan_off counts from wherever the caller counts: only its differences matter); n_msg: null without messages
    int build(lk_handle* h, const lk_point* d_pts, size_t n, size_t S, const uint64_t* scan_off, const double* t_begin, const uint32_t* n_msg) {
        h_so.resize(S + 1);
        for (size_t s = 0; s <= S; ++s) h_so[s] = scan_off[s] - scan_off[0];
        HIPCHK(h, hipMemcpyAsync(so, h_so.data(), 8 * (S + 1), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(t0, t_begin, 8 * S, hipMemcpyHostToDevice, h->stream));
        if (n_msg) {
            h_mo.assign(S + 1, 0);
            for (size_t s = 0; s < S; ++s) h_mo[s + 1] = h_mo[s] + n_msg[s];
            HIPCHK(h, hipMemcpyAsync(mo, h_mo.data(), 4 * (S + 1), hipMemcpyHostToDevice, h->stream));
        }
        HIPCHK(h, hipMemsetAsync(st, 0, 32, h->stream));
        const unsigned int nblk = (unsigned int)((n + 255) / 256);
        hipLaunchKernelGGL(lk_rag_flag_kernel, dim3(nblk), dim3(256), 0, h->stream, d_pts, (unsigned long long)n, so, (int)S, fl, st);
        size_t tmp_bytes = 0;
        HIPCHK(h, lk_prim_exclusive_scan(nullptr, tmp_bytes, fl, rk, n, h->stream));
        LKCHK(reserve(h, h->prim_tmp, tmp_bytes));
        HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, tmp_bytes, fl, rk, n, h->stream));
        hipLaunchKernelGGL(lk_rag_scatter_kernel, dim3(nblk), dim3(256), 0, h->stream, d_pts, (unsigned long long)n, so, (int)S, fl, rk, t0, ps, tb, bs, st);
        return LK_OK;
    }
};

// Body of the three entries: msgs is a host pointer, or a device pointer when msgs_on_device.
int replay_scans(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin, int msg_kind,
                 const uint32_t* n_msg, const void* msgs, bool msgs_on_device, lk_pose* out) {
    if (n_scans == 0 || n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans must be in [1, n_slots]");
    if (!d_pts || !scan_off || !t_begin) return fail(h, LK_ERR_INVALID, "null argument");
    if (msg_kind < 0 || msg_kind > 2 || (msg_kind && !n_msg)) return fail(h, LK_ERR_INVALID, "msg_kind must be 0 (none), 1 (lk_imu) or 2 (lk_kin_imu) with n_msg given");
    const size_t S = n_scans;
    if (scan_off[0] != 0) return fail(h, LK_ERR_INVALID, "scan_off[0] must be 0");
    for (size_t s = 0; s < S; ++s)
        if (scan_off[s + 1] <= scan_off[s]) return fail(h, LK_ERR_INVALID, "empty scan");
    const size_t n = scan_off[S];
    if (n >= ((size_t)1 << 32)) return fail(h, LK_ERR_CAPACITY, "more than 2^32 points in one batch");
    const size_t msg_bytes = msg_record_bytes(msg_kind);
    size_t n_msg_total = 0;
    if (msg_kind)
        for (size_t s = 0; s < S; ++s) n_msg_total += n_msg[s];
    if (n_msg_total && !msgs) return fail(h, LK_ERR_INVALID, "null message array");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    BucketTables bt;
    unsigned char* d_ms = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        bt.take(c, n, S);
        d_ms = c.take<unsigned char>(msg_bytes * n_msg_total);   // the messages
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->ragdev, bytes, bytes / 4));
    carve(h->ragdev.p);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "scan offsets are 64-bit");
    if (n_msg_total)
        HIPCHK(h, hipMemcpyAsync(d_ms, msgs, msg_bytes * n_msg_total, msgs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    LKCHK(bt.build(h, d_pts, n, S, scan_off, t_begin, msg_kind ? n_msg : nullptr));
    hipLaunchKernelGGL(lk_rag_stats_kernel, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, h->stream, bt.ps, bt.bs, (int)S, bt.st);
    HIPCHK(h, hipGetLastError());
    unsigned int st[4];
    HIPCHK(h, hipMemcpyAsync(st, bt.st, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const unsigned int biggest = st[1], most = st[2];
    if (st[3]) return fail(h, LK_ERR_INVALID, "a scan is not sorted by time (curvature must be non-decreasing within a scan, and finite)");
    if (biggest > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "bucket exceeds max_scan_points");
    if (msg_kind && biggest > (unsigned int)LK_SCAN_WAVE_MAX)
        return fail(h, LK_ERR_INVALID, "IMU / kinematic messages between buckets are only replayed for scans whose buckets hold <= 512 points");
    LkRagged rg;
    rg.pt_off = bt.ps;
    rg.t = bt.tb;
    rg.nb = nullptr;
    rg.ldb = (int)most;
    rg.bstart = bt.bs;
    rg.imu_off = msg_kind ? bt.mo : nullptr;
    rg.imu = reinterpret_cast<const double*>(d_ms);
    rag_from_handle(h, msg_kind, &rg);
    return ragged_launch(h, d_pts, S, rg, bt.t0, (int)biggest, (size_t)most, nullptr, msg_kind, out);
}

// Whole recorded runs, a run per filter slot (lk_batch_replay_overlay_runs_dev with the insert, lk_batch_replay_runs_dev on the frozen map): run r = the
// scans run_off[r] .. run_off[r+1) on slot r.  Bucket tables: built for all scans at once (BucketTables, CSR), in which a run is one contiguous bucket
// range - the launches replay it as one long scan whose kernels know where its scans end (LkRagged::run_scan).  What the two entries share comes in two
// halves, so that an entry can put checks of its own between them: runs_check() is everything the host can refuse from the arguments alone,
// RunBatch::build() the tables on the device and what they say about the scans.  Nothing here writes to a filter slot.
struct RunBatch {
    size_t R = 0, S = 0, n = 0, max_run_pts = 0;   // runs, scans, points; the most points of a run
    LkRagged rg;                                   // the runs' tables: bstart = the runs' first buckets, ldb = most buckets of a run
    const double* d_rt = nullptr;                  // [R] the runs' start times
    unsigned int biggest = 0, most_run = 0;        // largest bucket (points), most buckets of a run
    unsigned int n_buckets = 0;                    // flat buckets of the batch
    std::vector<uint32_t> h_bs;                    // the scans' first flat buckets, [S + 1] (record(): the _cloud entries)
    int record(lk_handle* h, bool on);
    int finish(lk_handle* h, const lk_point* d_pts, float* d_world_out, uint32_t* scan_bucket_off);
    int build(lk_handle* h, const lk_point* d_pts, const uint32_t* run_off, const uint64_t* scan_off, const double* t_begin, int msg_kind, const uint32_t* n_msg,
              const void* d_msgs);
};
static int runs_check(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off, const double* t_begin, int msg_kind,
                      const uint32_t* n_msg, const void* d_msgs, RunBatch* rb) {
    if (n_runs == 0 || n_runs > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_runs must be in [1, n_slots]");
    if (!d_pts || !run_off || !scan_off || !t_begin) return fail(h, LK_ERR_INVALID, "null argument");
    if (msg_kind < 0 || msg_kind > 2 || (msg_kind && !n_msg)) return fail(h, LK_ERR_INVALID, "msg_kind must be 0 (none), 1 (lk_imu) or 2 (lk_kin_imu) with n_msg given");
    const size_t R = n_runs;
    if (run_off[0] != 0) return fail(h, LK_ERR_INVALID, "run_off[0] must be 0");
    for (size_t r = 0; r < R; ++r)
        if (run_off[r + 1] <= run_off[r]) return fail(h, LK_ERR_INVALID, "run " + std::to_string(r) + " is empty");
    const size_t S = run_off[R];
    if (scan_off[0] != 0) return fail(h, LK_ERR_INVALID, "scan_off[0] must be 0");
    size_t n_msg_total = 0;
    for (size_t s = 0; s < S; ++s) {
        if (scan_off[s + 1] <= scan_off[s]) return fail(h, LK_ERR_INVALID, "scan " + std::to_string(s) + " is empty");
        if (msg_kind) n_msg_total += n_msg[s];
    }
    const size_t n = scan_off[S];
    if (n >= ((size_t)1 << 32)) return fail(h, LK_ERR_CAPACITY, "more than 2^32 points in one batch");
    if (n_msg_total && !d_msgs) return fail(h, LK_ERR_INVALID, "null message array");
    if (n_msg_total >= ((size_t)1 << 32)) return fail(h, LK_ERR_CAPACITY, "more than 2^32 messages in one batch");
    rb->R = R, rb->S = S, rb->n = n, rb->max_run_pts = 0;
    for (size_t r = 0; r < R; ++r) rb->max_run_pts = std::max(rb->max_run_pts, (size_t)(scan_off[run_off[r + 1]] - scan_off[run_off[r]]));
    return LK_OK;
}
int RunBatch::build(lk_handle* h, const lk_point* d_pts, const uint32_t* run_off, const uint64_t* scan_off, const double* t_begin, int msg_kind, const uint32_t* n_msg,
                    const void* d_msgs) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    BucketTables bt;
    unsigned int *d_ro = nullptr, *d_rb = nullptr;
    double* rt = nullptr;
    lk_pose* d_pose = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        bt.take(c, n, S);
        d_ro = c.take<unsigned int>(R + 1), d_rb = c.take<unsigned int>(R + 1);   // the runs' first scans, their first buckets
        rt = c.take<double>(R);                                                    // their start times
        d_pose = c.take<lk_pose>(S);
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->ragdev, bytes, bytes / 4));
    carve(h->ragdev.p);
    HIPCHK(h, hipMemcpyAsync(d_ro, run_off, 4 * (R + 1), hipMemcpyHostToDevice, h->stream));
    LKCHK(bt.build(h, d_pts, n, S, scan_off, t_begin, msg_kind ? n_msg : nullptr));
    hipLaunchKernelGGL(lk_rag_stats_kernel, dim3((unsigned int)((std::max(n, S) + 255) / 256)), dim3(256), 0, h->stream, bt.ps, bt.bs, (int)S, bt.st);
    hipLaunchKernelGGL(lk_rag_run_tables_kernel, dim3((unsigned int)((R + 256) / 256)), dim3(256), 0, h->stream, bt.bs, d_ro, bt.t0, (int)R, d_rb, rt, bt.st);
    HIPCHK(h, hipGetLastError());
    unsigned int st[8];
    HIPCHK(h, hipMemcpyAsync(st, bt.st, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    biggest = st[1], most_run = st[5], n_buckets = st[0];
    if (st[3])
        return fail(h, LK_ERR_INVALID, "scan " + std::to_string(S - st[3]) + " is not sorted by time (curvature must be non-decreasing within a scan, and finite)");
    if (biggest > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "bucket exceeds max_scan_points");
    rg.pt_off = bt.ps;
    rg.t = bt.tb;
    rg.nb = nullptr;
    rg.ldb = (int)most_run;
    rg.bstart = d_rb;
    rg.imu_off = msg_kind ? bt.mo : nullptr;
    rg.imu = reinterpret_cast<const double*>(d_msgs);   // read where they lie
    rag_from_handle(h, msg_kind, &rg);
    rg.run_scan = d_ro, rg.scan_b = bt.bs, rg.scan_pose = d_pose;
    d_rt = rt;
    return LK_OK;
}
// The _cloud entries, ahead of the launches (and behind every refusal the host can make): room for the batch's bucket records in the handle's table, which
// the kernels then fill (LkRagged::bucket_pose), and the scans' first buckets for scan_bucket_off.  A table that has to grow loses its old records.
int RunBatch::record(lk_handle* h, bool on) {
    if (!on) return LK_OK;
    const size_t bytes = lk_cloud_table_bytes(n_buckets, sizeof(lk_bucket_pose));
    if (bytes > h->bucket_tab.cap) h->bucket_n = 0;
    LKCHK(reserve(h, h->bucket_tab, bytes, bytes / 4));
    rg.bucket_pose = static_cast<lk_bucket_pose*>(h->bucket_tab.p);
    h_bs.resize(S + 1);
    HIPCHK(h, hipMemcpyAsync(h_bs.data(), rg.scan_b, 4 * (S + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
// ... and behind a replay that has succeeded: the table is the handle's last recording, the scans' ranges in it go to the caller, and the cloud - every
// point under its bucket's record - is one launch on the handle's stream (not made without d_world_out).
int RunBatch::finish(lk_handle* h, const lk_point* d_pts, float* d_world_out, uint32_t* scan_bucket_off) {
    if (!rg.bucket_pose) return LK_OK;
    if (lk_cloud_scan_offsets(h_bs.data(), S, scan_bucket_off) != (uint64_t)n_buckets) return fail(h, LK_ERR_STATE, "bucket tables: the scans' first buckets do not add up");
    h->bucket_n = n_buckets;
    if (!d_world_out) return LK_OK;
    LAUNCH(h, "register_cloud", hipLaunchKernelGGL(lk_register_cloud_kernel, dim3(lk_cloud_tiles(n)), dim3(LK_REG_TILE), 0, h->stream, d_pts, (unsigned long long)n,
                                                   rg.pt_off, n_buckets, rg.bucket_pose, h->pr, d_world_out));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
static int cloud_args_check(lk_handle* h, const float* d_world_out) {
    if ((uintptr_t)d_world_out & 15u) return fail(h, LK_ERR_INVALID, "d_world_out must be 16-byte aligned");
    return LK_OK;
}

// Batch replay WITH insert of whole recorded runs: run r = the scans run_off[r] .. run_off[r+1) on filter slot r, each scan what
// lk_batch_replay_overlay_ragged_dev does for one - but the slot's state, covariance, times and overlay survive the scan boundary, as KILO's members do
// from one KILO::process to the next, and the message cursor jumps to the next scan's first record (what a package left over is never applied).
// out[s]: the pose after scan s, its counters that scan's alone.
int lk_batch_replay_overlay_runs_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off,
                                     const double* t_begin, int msg_kind, const uint32_t* n_msg, const void* d_msgs, lk_pose* out) {
    return lk_batch_replay_overlay_runs_cloud_dev(h, d_pts, n_runs, run_off, scan_off, t_begin, msg_kind, n_msg, d_msgs, out, nullptr, nullptr);
}
// ... with the state behind every bucket recorded in the handle's bucket table (either output given) and the scans registered under those states
// (d_world_out): RunBatch::record / finish.  With both NULL this is the entry above, kernel for kernel.
int lk_batch_replay_overlay_runs_cloud_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off,
                                           const double* t_begin, int msg_kind, const uint32_t* n_msg, const void* d_msgs, lk_pose* out,
                                           float* d_world_out, uint32_t* scan_bucket_off) {
    CHECK_H(h);
    LKCHK(cloud_args_check(h, d_world_out));
    RunBatch rb;
    LKCHK(runs_check(h, d_pts, n_runs, run_off, scan_off, t_begin, msg_kind, n_msg, d_msgs, &rb));
    LkMap fmap;   // (asked here, ahead of the tables: a handle without the grid is refused before anything is built)
    LKCHK(frozen_map(h, &fmap));
    if (!fmap.grid_on) return fail(h, LK_ERR_STATE, "overlay replay needs the frozen-map grid (root keys' bounding box too large, LEGKILO_GRID=0, or out of device memory)");
    LKCHK(rb.build(h, d_pts, run_off, scan_off, t_begin, msg_kind, n_msg, d_msgs));
    LKCHK(rb.record(h, d_world_out || scan_bucket_off));
    LKCHK(overlay_ragged_launch(h, d_pts, rb.R, rb.rg, rb.d_rt, (int)rb.biggest, (size_t)rb.most_run, nullptr, rb.max_run_pts, msg_kind, out, rb.S));
    return rb.finish(h, d_pts, d_world_out, scan_bucket_off);
}

// The same runs on the FROZEN map - no insert, no overlay, the handle's map unchanged: per scan what lk_batch_replay_scans_dev does for one (grid if
// there is one, hash otherwise), state, covariance and both time stamps carried across the scan boundaries, the message cursor as above.  On a frozen
// map a slot's filter record is the whole carried state: with LK_RUNS_CONTINUE the slots go on from what they hold (no reset of the times), so a run
// split at any scan boundary into consecutive calls gives the bits of one call.  Every check comes before the first write to a slot.
int lk_batch_replay_runs_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off, const double* t_begin,
                             int msg_kind, const uint32_t* n_msg, const void* d_msgs, uint32_t flags, lk_pose* out) {
    return lk_batch_replay_runs_cloud_dev(h, d_pts, n_runs, run_off, scan_off, t_begin, msg_kind, n_msg, d_msgs, flags, out, nullptr, nullptr);
}
int lk_batch_replay_runs_cloud_dev(lk_handle* h, const lk_point* d_pts, size_t n_runs, const uint32_t* run_off, const uint64_t* scan_off, const double* t_begin,
                                   int msg_kind, const uint32_t* n_msg, const void* d_msgs, uint32_t flags, lk_pose* out, float* d_world_out,
                                   uint32_t* scan_bucket_off) {
    CHECK_H(h);
    LKCHK(cloud_args_check(h, d_world_out));
    if (flags & ~LK_RUNS_CONTINUE) return fail(h, LK_ERR_INVALID, "unknown flag bits (LK_RUNS_CONTINUE is the only one)");
    RunBatch rb;
    LKCHK(runs_check(h, d_pts, n_runs, run_off, scan_off, t_begin, msg_kind, n_msg, d_msgs, &rb));
    LKCHK(rb.build(h, d_pts, run_off, scan_off, t_begin, msg_kind, n_msg, d_msgs));
    if (msg_kind && rb.biggest > (unsigned int)LK_SCAN_WAVE_MAX)
        return fail(h, LK_ERR_INVALID, "IMU / kinematic messages between buckets are only replayed for scans whose buckets hold <= 512 points");
    LKCHK(rb.record(h, d_world_out || scan_bucket_off));
    LKCHK(ragged_launch(h, d_pts, rb.R, rb.rg, (flags & LK_RUNS_CONTINUE) ? nullptr : rb.d_rt, (int)rb.biggest, (size_t)rb.most_run, nullptr, msg_kind, out, rb.S));
    return rb.finish(h, d_pts, d_world_out, scan_bucket_off);
}
// Records first_bucket .. first_bucket + n of the table the handle's last batch replay recorded (a _cloud run replay; anything else records nothing).
static int bucket_poses_copy(lk_handle* h, uint64_t first_bucket, size_t n, lk_bucket_pose* out, hipMemcpyKind kind) {
    if (!h->bucket_n) return fail(h, LK_ERR_STATE, "the handle's last batch replay recorded no bucket poses (lk_batch_replay_runs_cloud_dev / lk_batch_replay_overlay_runs_cloud_dev do)");
    if (!lk_cloud_range_ok(first_bucket, n, h->bucket_n)) return fail(h, LK_ERR_INVALID, "bucket range ends past the " + std::to_string(h->bucket_n) + " records of the table");
    if (n == 0) return LK_OK;
    if (!out) return fail(h, LK_ERR_INVALID, "null argument");
    HIPCHK(h, hipMemcpyAsync(out, static_cast<const lk_bucket_pose*>(h->bucket_tab.p) + first_bucket, sizeof(lk_bucket_pose) * n, kind, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_runs_bucket_poses_dev(lk_handle* h, uint64_t first_bucket, size_t n, lk_bucket_pose* d_out) {
    CHECK_H(h);
    return bucket_poses_copy(h, first_bucket, n, d_out, hipMemcpyDeviceToDevice);
}
int lk_runs_bucket_poses(lk_handle* h, uint64_t first_bucket, size_t n, lk_bucket_pose* out) {
    CHECK_H(h);
    return bucket_poses_copy(h, first_bucket, n, out, hipMemcpyDeviceToHost);
}

// The tables of a live run (RunTables): the same CSR tables over the run's points - d_pts is the run's FIRST point - followed by the per-scan
// summaries.  Nothing of the handle but scratch is touched.
int run_tables(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin, const uint32_t* n_msg, RunTables* out) {
    const size_t S = n_scans, n = scan_off[S] - scan_off[0];
    if (n >= ((size_t)1 << 32)) return fail(h, LK_ERR_CAPACITY, "more than 2^32 points in one run");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    BucketTables bt;
    unsigned int *d_sum = nullptr, *d_nbp = nullptr, *d_sync = nullptr;
    int* d_rs = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        bt.take(c, n, S);
        d_sum = c.take<unsigned int>(4 * S), d_nbp = c.take<unsigned int>(2 * S); // per-scan summaries, { buckets, 0 } pairs
        d_sync = c.take<unsigned int>(4 * S), d_rs = c.take<int>(8 * S);          // per-scan barrier words, LkResume
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->ragdev, bytes, bytes / 4));
    carve(h->ragdev.p);
    HIPCHK(h, hipMemsetAsync(d_sync, 0, 16 * S, h->stream));
    LKCHK(bt.build(h, d_pts, n, S, scan_off, t_begin, n_msg));
    hipLaunchKernelGGL(lk_rag_scan_summary_kernel, dim3((unsigned int)((S + 3) / 4)), dim3(256), 0, h->stream, bt.ps, bt.bs, n_msg ? bt.mo : (unsigned int*)nullptr,
                       (int)S, bt.st, d_sum, d_nbp, d_rs);
    HIPCHK(h, hipGetLastError());
    unsigned int st[8];
    out->bstart.resize(S + 1), out->sum.resize(4 * S);
    HIPCHK(h, hipMemcpyAsync(st, bt.st, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out->bstart.data(), bt.bs, 4 * (S + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out->sum.data(), d_sum, 16 * S, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out->first_unsorted = st[4];
    out->d_ps = bt.ps, out->d_tb = bt.tb, out->d_nbp = d_nbp, out->d_mo = n_msg ? bt.mo : nullptr, out->d_sync = d_sync, out->d_resume = d_rs;
    return LK_OK;
}

// Asynchronous, double-buffered batch replay.  The batch uses filter slots [first_slot, first_slot + n_scans); calls whose
// slot ranges alternate (first_slot = 0, n_scans, 0, ...) run on alternate HIP streams, so the single-workgroup update /
// predict kernels of one batch overlap the full-size residual launches of the next instead of sitting between them.
// Everything of a batch - arming the priors (d_x36 / d_P900 may be NULL: keep the slots' current state), the bucket
// chain, the pose gather and its copy to (pinned) host memory - is stream-ordered on the batch's own stream; nothing
// synchronises.  lk_synchronize() waits for all streams.
int lk_batch_replay_async_dev(lk_handle* h, const lk_point* d_pts, uint32_t first_slot, size_t n_scans, size_t n_pts, double t_begin,
                              const uint32_t* bucket_off, const double* bucket_dt, size_t n_buckets, const double* d_x36,
                              const double* d_P900, lk_pose* host_out) {
    CHECK_H(h);
    if (n_scans == 0 || (size_t)first_slot + n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "slot range must lie in [0, n_slots]");
    if (n_pts == 0 || n_buckets == 0) return fail(h, LK_ERR_INVALID, "empty scans");
    if (!d_pts || !bucket_off || !bucket_dt) return fail(h, LK_ERR_INVALID, "null argument");
    if ((d_x36 == nullptr) != (d_P900 == nullptr)) return fail(h, LK_ERR_INVALID, "give both prior buffers or neither");
    const int S = (int)n_scans;
    std::vector<size_t> live;
    LKCHK(live_buckets(h, bucket_off, n_buckets, live));   // all checks before the first enqueue
    LkMap fmap;
    LKCHK(frozen_map(h, &fmap));   // synchronises once per map snapshot (grid rebuild), otherwise free
    // batches on slot ranges 0, n, 2n, ... rotate over up to three streams (the handle's + two side streams): with three batches in
    // flight there is (almost) always a residual launch ready while the other two sit in their update / predict launches
    // The stream is a function of (first_slot, n_scans): two batches in flight on overlapping slots are ordered only if they
    // share it.  So first_slot must be a multiple of n_scans (slot ranges of one size never overlap partially), and when the batch
    // size changes while batches may still be in flight the streams are drained first.
    if (first_slot % (uint32_t)n_scans != 0) return fail(h, LK_ERR_INVALID, "first_slot must be a multiple of n_scans");
    if (h->async_n != 0 && h->async_n != n_scans) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i)
            if (h->side[i]) HIPCHK(h, hipStreamSynchronize(h->side[i]));
    }
    h->async_n = n_scans;
    h->bucket_n = 0;
    const uint32_t ring = (first_slot / (uint32_t)n_scans) % 3u;
    hipStream_t st = ring == 0 ? h->stream : h->side[ring - 1];
    LkFilter* fl = h->d_filters + first_slot;
    if (st != h->stream && !d_x36) {
        // the slots' state was armed elsewhere (lk_batch_set_priors_dev is asynchronous on the MAIN stream): order this batch
        // after it.  With d_x36 / d_P900 the batch arms its own slots on its own stream and needs no such edge - which is
        // what keeps two batches in flight.
        HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
        HIPCHK(h, hipStreamWaitEvent(st, h->ev_fork, 0));
    }
    if (d_x36) {
        HIPCHK(h, hipMemcpy2DAsync(fl[0].x, sizeof(LkFilter), d_x36, sizeof(double) * 36, sizeof(double) * 36, n_scans, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpy2DAsync(fl[0].P, sizeof(LkFilter), d_P900, sizeof(double) * 900, sizeof(double) * 900, n_scans, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(h, hipMemset2DAsync(&fl[0].n_effect, sizeof(LkFilter), 0, 24, n_scans, st));
    hipLaunchKernelGGL(lk_set_times_kernel, dim3((S + 63) / 64), dim3(64), 0, st, fl, S, t_begin);
    ResidualOut ro;
    memset(&ro, 0, sizeof(ro));
    LKCHK(batch_ordered(h, d_pts, first_slot, n_scans, n_pts, bucket_off, n_buckets, st, ring, &ro));   // first sight of a batch synchronises; afterwards one small launch
    LKCHK(enqueue_frozen_chain(h, st, false, first_slot, S, d_pts, ro.alt_pts, n_pts, live, bucket_off, bucket_dt, t_begin, fmap, ro));
    if (host_out) {
        hipLaunchKernelGGL(lk_pose_gather_kernel, dim3((S + 63) / 64), dim3(64), 0, st, fl, h->d_poses + first_slot, S);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(host_out, h->d_poses + first_slot, sizeof(lk_pose) * n_scans, hipMemcpyDeviceToHost, st));
    }
    return LK_OK;
}

// ------------------------------------------------------------------ measurement hooks
int lk_profile_enable(lk_handle* h, int on) {
    CHECK_H(h);
    h->profiling = on != 0;
    return LK_OK;
}
int lk_profile_get(lk_handle* h, const char* kernel, uint64_t* launches, double* total_ms) {
    CHECK_H(h);
    auto it = h->prof.find(kernel ? kernel : "");
    if (it == h->prof.end()) {
        if (launches) *launches = 0;
        if (total_ms) *total_ms = 0.0;
        return LK_OK;
    }
    if (launches) *launches = it->second.launches;
    if (total_ms) *total_ms = it->second.total_ms;
    return LK_OK;
}
int lk_profile_reset(lk_handle* h) {
    CHECK_H(h);
    h->prof.clear();
    return LK_OK;
}
int lk_device_malloc(lk_handle* h, void** d_ptr, size_t bytes) {
    CHECK_H(h);
    HIPCHK(h, hipMalloc(d_ptr, bytes));
    return LK_OK;
}
int lk_device_free(lk_handle* h, void* d_ptr) {
    CHECK_H(h);
    HIPCHK(h, hipFree(d_ptr));
    return LK_OK;
}
int lk_memcpy_h2d(lk_handle* h, void* d_dst, const void* src, size_t bytes) {
    CHECK_H(h);
    HIPCHK(h, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_memcpy_d2h(lk_handle* h, void* dst, const void* d_src, size_t bytes) {
    CHECK_H(h);
    HIPCHK(h, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
int lk_synchronize(lk_handle* h) {
    CHECK_H(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < lk_handle::kMaxGroups - 1; ++i)
        if (h->side[i]) HIPCHK(h, hipStreamSynchronize(h->side[i]));  // double-buffered async batches live there
    h->async_n = 0;
    return LK_OK;
}
int lk_stream_pipeline(lk_handle* h, int on) {
    CHECK_H(h);   // joins the inserts in flight
    h->spec_enable = on != 0;
    return LK_OK;
}
int lk_stream_resident(lk_handle* h, int on) {
    CHECK_H(h);
    h->resident_enable = on != 0;
    return LK_OK;
}
int lk_stream_grid(lk_handle* h, int on) {
    CHECK_H(h);
    h->gridscan_mode = std::min(std::max(on, 0), 2);
    return LK_OK;
}
int lk_test_stall(lk_handle* h, unsigned int bound_ms) {
    CHECK_H(h);
    h->test_stall_ms = bound_ms & 0x7fffffffu;
    return LK_OK;
}
int lk_stream_resident_stats(lk_handle* h, uint64_t* out2) {
    CHECK_H(h);
    if (!out2) return fail(h, LK_ERR_INVALID, "out2 is null");
    out2[0] = h->resident_scans + h->grid_scans, out2[1] = h->resident_relaunches + h->grid_relaunches;
    return LK_OK;
}
int lk_stream_stats(lk_handle* h, uint64_t* out4) {
    CHECK_H(h);
    if (!out4) return fail(h, LK_ERR_INVALID, "out4 is null");
#ifdef LK_DEBUG_LI
    {
        unsigned long long hb[64];
        hipStreamSynchronize(h->stream);
        hipMemcpyFromSymbol(hb, HIP_SYMBOL(lk_li_dbg), sizeof(hb));
        fprintf(stderr, "[li] %llu mismatches, %llu traced\n", hb[0], hb[60]);
        for (int k = 0; k < 4 && k < (int)hb[60]; ++k) {
            const unsigned long long* o = hb + 1 + 14 * k;
            fprintf(stderr, "[tr] leaf %d root %d Tn %d Tp %d To %d g %d r.npts %d r.block %d layer %d newp %d state %llx consumed %d need_init %d off %d\n", (int)o[0], (int)o[1],
                    (int)o[2], (int)o[3], (int)o[4], (int)o[5], (int)o[6], (int)o[7], (int)o[8], (int)o[9], o[10], (int)o[11], (int)o[12], (int)o[13]);
        }
        for (int k = 0; k < 4 && k < (int)hb[0]; ++k) {
            const unsigned long long* o = hb + 1 + 14 * k;
            fprintf(stderr, "[li] leaf %lld root %lld npts %d/%d newp %d/%d block %d/%d layer %lld/%lld state %llx/%llx plane %lld off %lld\n", (long long)o[0], (long long)o[1],
                    (int)o[2], (int)o[3], (int)o[4], (int)o[5], (int)o[6], (int)o[7], (long long)o[8], (long long)o[9], o[10], o[11], (long long)o[12], (long long)o[13]);
        }
    }
#endif
#ifdef LK_DEBUG_INS
    {
        unsigned long long hb[16];
        unsigned int ctr[LK_CTR_COUNT];
        hipStreamSynchronize(h->stream);
        hipMemcpyFromSymbol(hb, HIP_SYMBOL(lk_ins_dbg), sizeof(hb));
        hipMemcpy(ctr, h->map.counters, sizeof(ctr), hipMemcpyDeviceToHost);
        const char* names[8] = {"desc+node", "points", "simulate", "stores", "eigen", "plane_var", "commit", "tail"};
        fprintf(stderr, "[ins] %llu groups, %llu fitted; per group (us):", hb[15], hb[14]);
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %s %.2f;", names[k], (double)hb[k] / (double)(hb[15] ? hb[15] : 1) * 0.01);
        fprintf(stderr, " block-load wait %.2f;", (double)hb[8] / (double)(hb[15] ? hb[15] : 1) * 0.01);
        { unsigned long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(lk_ins_dbg), z, sizeof(z)); }
        fprintf(stderr, "\n[ins] plane_var: %.0f shader cycles and %.2f us per fit -> %.2f GHz", (double)hb[12] / (double)(hb[14] ? hb[14] : 1),
                (double)hb[13] / (double)(hb[14] ? hb[14] : 1) * 0.01, (double)hb[12] / ((double)hb[13] * 10.0 + 1e-9));
        fprintf(stderr, "\n[ins] last bucket: touched %u heavy %u groups %u gidx %u fallback %u\n", ctr[LK_CTR_TOUCHED], ctr[LK_CTR_HEAVY],
                ctr[LK_CTR_GROUPS], ctr[LK_CTR_GIDX], ctr[LK_CTR_FALLBACK]);
        unsigned int rh[6 * 32];
        hipMemcpyFromSymbol(rh, HIP_SYMBOL(lk_root_hist), sizeof(rh));
        const char* rows[6] = {"light", "one group", "several groups", "long", "wave before 2nd root", "load+sort+walk"};
        for (int r = 0; r < 6; ++r) {
            fprintf(stderr, "[root] %-22s 2-us bins:", rows[r]);
            for (int b = 0; b < 32; ++b) fprintf(stderr, " %u", rh[r * 32 + b]);
            fprintf(stderr, "\n");
        }
        memset(rh, 0, sizeof(rh));
        hipMemcpyToSymbol(HIP_SYMBOL(lk_root_hist), rh, sizeof(rh));
        {
            unsigned long long sd[32];
            hipMemcpyFromSymbol(sd, HIP_SYMBOL(lk_slow_dbg), sizeof(sd));
            const char* pn[10] = {"desc+node", "points", "simulate", "stores", "eigen", "plane_var", "commit", "tail", "block-load", "-"};
            for (int w = 0; w < 2; ++w) {
                fprintf(stderr, "[apply] plane-fit groups %s 20 us: %llu; per group (us):", w == 0 ? ">=" : "<", sd[16 * w + 15]);
                for (int k = 0; k < 9; ++k) fprintf(stderr, " %s %.2f;", pn[k], (double)sd[16 * w + k] / (double)(sd[16 * w + 15] ? sd[16 * w + 15] : 1) * 0.01);
                fprintf(stderr, "\n");
            }
            memset(sd, 0, sizeof(sd));
            hipMemcpyToSymbol(HIP_SYMBOL(lk_slow_dbg), sd, sizeof(sd));
        }
        unsigned int eh[16 * 32];
        hipMemcpyFromSymbol(eh, HIP_SYMBOL(lk_ev_hist), sizeof(eh));
        for (int r = 0; r < 16; ++r) {
            fprintf(stderr, "[apply] flags %2d (1 new child, 2 new block, 4 frozen, 8 plane fit) 2-us bins:", r);
            for (int b = 0; b < 32; ++b) fprintf(stderr, " %u", eh[r * 32 + b]);
            fprintf(stderr, "\n");
        }
        memset(eh, 0, sizeof(eh));
        hipMemcpyToSymbol(HIP_SYMBOL(lk_ev_hist), eh, sizeof(eh));
    }
#endif
    unsigned int redo[3] = {0, 0, 0};   // LK_CTR_SPEC_REDO, [13], LK_CTR_RES_REDO
    HIPCHK(h, hipMemcpyAsync(redo, h->map.counters + LK_CTR_SPEC_REDO, sizeof(redo), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (redo[0] < h->spec_redo_seen) h->spec_redo_seen = 0;          // the device words are reset with the pools (map import)
    h->spec_redo_total += (uint64_t)(redo[0] - h->spec_redo_seen);
    h->spec_redo_seen = redo[0];
    if (redo[2] < h->res_redo_seen) h->res_redo_seen = 0;
    h->res_redo_total += (uint64_t)(redo[2] - h->res_redo_seen);
    h->res_redo_seen = redo[2];
    out4[0] = h->spec_buckets, out4[1] = h->spec_tiles, out4[2] = h->spec_redo_total, out4[3] = h->res_redo_total;
    return LK_OK;
}
int lk_stream_grid_placement(lk_handle* h, uint32_t* xcc_mask) {
    CHECK_H(h);
    if (!xcc_mask) return fail(h, LK_ERR_INVALID, "xcc_mask is null");
    HIPCHK(h, hipMemcpyAsync(xcc_mask, h->map.counters + LK_CTR_GRID_XCC, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
void* lk_stream(lk_handle* h) { return h ? (void*)h->stream : nullptr; }

}  // extern "C"
