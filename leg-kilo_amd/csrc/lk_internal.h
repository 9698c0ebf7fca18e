// lk_internal.h - what the translation units of liblegkilo_hip.so share: the handle, the error / launch / allocation helpers, and the kernel
// headers.  The library is nine units compiled side by side - legkilo_hip.hip (LK_TU_MAIN: the C-ABI but for the overlay entries, and every
// kernel but the overlay's and the stream path's own), lk_stream.hip (LK_TU_STREAM: one live scan after the other with the map insert - the per-bucket
// launches, the scan-resident / grid-resident / pipelined kernels, and the KILO-path entries, which all run a scan through run_one_scan: one choice of its kernel), lk_overlay.hip (LK_TU_OVERLAY: batch replay
// WITH insert - lk_overlay_kernels.h's kernels and the entries that launch them, lk_overlay_commit among them: its compaction steps, MapCompact below, are the main unit's), lk_ovscan.hip (LK_TU_OVSCAN: that replay's scan-resident kernel for small buckets), lk_ovrun.hip (the same file's run-resident instantiations), lk_kin.hip (LK_TU_KIN: the message front ends - HighState decode + contact detector, lk_kin_kernels.h; sensor_msgs/Imu decode, lk_imu_kernels.h; the scan split of either - and their entries), lk_traj.hip (LK_TU_TRAJ: trajectory error against ground truth, absolute and relative, lk_traj_kernels.h, and its four entries behind one host path), lk_c2c.hip (LK_TU_C2C: the map-cloud scores - cloud-to-cloud distance, lk_c2c_kernels.h, and map entropy / plane variance, lk_mme_kernels.h, both compiled in that unit only - and their four entries, the host ones through one staging helper), lk_prim.hip (rocPRIM).  A non-template kernel of a shared header is DEFINED in the main unit; the overlay unit sees its prototype
// (LK_KERNELS_ELSEWHERE) and launches it through the main unit's host stub.  The overlay header's own kernels are compiled in the overlay unit only.
#pragma once
#if !defined(LK_TU_MAIN) && !defined(LK_TU_OVERLAY) && !defined(LK_TU_STREAM) && !defined(LK_TU_OVSCAN) && !defined(LK_TU_KIN) && !defined(LK_TU_TRAJ) && !defined(LK_TU_C2C)
#error "define LK_TU_MAIN, LK_TU_STREAM, LK_TU_OVERLAY, LK_TU_OVSCAN, LK_TU_KIN, LK_TU_TRAJ or LK_TU_C2C before including lk_internal.h"
#endif
#if defined(LK_TU_OVERLAY) || defined(LK_TU_STREAM) || defined(LK_TU_OVSCAN) || defined(LK_TU_KIN) || defined(LK_TU_TRAJ) || defined(LK_TU_C2C)
#define LK_KERNELS_ELSEWHERE 1
#endif
// legkilo_hip.hip — implementation of the C-ABI in include/legkilo_hip.h for gfx950.
// Host side of the shim: owns HBM pools, the HIP stream, and the launch sequences that
// replace KILO::predictUpdatePoint (KILO.cc:108-233) and the bucket loop (KILO.cc:367-396).
// There is no CPU fallback: without a gfx950 device lk_create fails with LK_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "lk_carve.h"  // one buffer carved into typed arrays
#include "lk_prim.h"   // rocPRIM's sorts and scans, instantiated in lk_prim.hip

#include "lk_device.h"
#include "lk_filter_kernels.h"
#include "lk_point_kernels.h"
#include "lk_map_kernels.h"
#ifdef LK_TU_MAIN
#include "lk_pre_kernels.h"   // decode / voxel grid / ragged tables: launched by the main unit only
#include "lk_query_kernels.h" // per-point build_single_residual: launched by the main unit only
#include "lk_mapcloud_kernels.h" // voxel grid over files of registered points (lk_downsample_clouds_dev): launched by the main unit only
#endif
#include "lk_overlay_kernels.h"

static_assert(sizeof(lk_plane_rec) == 256, "plane record must be 256 B");
static_assert(sizeof(lk_node_rec) == 128, "node record must be 128 B");
static_assert(sizeof(lk_pt_rec) == 72, "point record must be 72 B");
static_assert(sizeof(lk_point) == 16, "scan point must be 16 B");
static_assert(sizeof(lk_bucket_pose) == 144, "bucket record must be 144 B");

struct ProfEntry {
    uint64_t launches = 0;
    double total_ms = 0.0;
};

// Device memory that belongs to the handle, grows on demand and never shrinks (reserve() below; `pinned`: page-locked host memory instead).
// A new scratch buffer is one DevBuf member of lk_handle and one reserve() where it is used: lk_destroy frees whatever was reserved.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;        // bytes
    bool pinned = false;
    bool listed = false;   // in lk_handle::grown
};

struct lk_handle {
    lk_config cfg = {};
    LkParams pr = {};
    LkMap map = {};
    hipStream_t stream = nullptr;
    static constexpr int kMaxGroups = 4;
    hipStream_t side[kMaxGroups - 1] = {};  // extra queues of the slot-group batch replay
    hipEvent_t ev_fork = nullptr, ev_join[kMaxGroups - 1] = {};
    int replay_groups = 3;
    size_t async_n = 0;           // n_scans of the asynchronous batches that may be in flight (0: none since the last lk_synchronize)
    bool wave_update = true;  // batch replay: single-wave update kernel (LEGKILO_UPDATE_CLASSIC=1 selects the 256-thread one)
    double last_slide_position[3] = {0.0, 0.0, 0.0};  // voxel_map.h:201
    unsigned int hash_cap = 0;
    LkFilter* d_filters = nullptr;
    double* d_Q = nullptr;
    double* d_partials = nullptr;
    size_t part_stride = 0;  // doubles per slot
    lk_point* d_scan = nullptr;
    float* d_world = nullptr;
    double* d_rows = nullptr;  // h6 (6n) | z (n) | R (n)
    unsigned char* d_valid = nullptr;
    double* d_tmp = nullptr;   // small scratch for class-surface calls (>= 18*32 doubles + 900*2)
    lk_pose* d_poses = nullptr;
    // what lk_destroy frees: the fixed pools as pool_alloc handed them out, the grow-only buffers that reserve() has allocated
    std::vector<void*> pools;
    std::vector<DevBuf*> grown;
    DevBuf prim_tmp;              // temporary storage of every rocPRIM call (all of them run on `stream`)
    DevBuf ragdev;                // lk_batch_replay_scans_dev: flags, ranks, CSR tables, messages
    DevBuf rag, rag_stage{nullptr, 0, true};   // tables of lk_batch_replay_ragged_dev and of the resident stream kernels: device copy, pinned staging copy (rag_reserve)
    // pipelined stream path ("spec"): the insert of bucket k on its own stream beside predict + residual of bucket k+1 (enqueue_bucket)
    hipStream_t ins = nullptr;
    hipEvent_t ev_U[2] = {}, ev_D[2] = {}, ev_I = nullptr;
    unsigned int epoch = 16;      // bucket sequence number: stamps of LkMap::dirty / newroot, value of spec[LK_SPEC_DONE]
    unsigned int spec_base = 16;  // first epoch of the open window (stamps below it belong to inserts that were joined)
    bool spec_open = false;       // inserts may still be running on `ins`
    int gridscan_mode = 1;        // scans of large buckets as one grid-resident launch (lk_scan_grid_kernel): 0 never, 1 when every bucket holds
                                  // 513 .. LK_GRIDSCAN_AUTO_MAX points (where it measures faster than the launches), 2 whenever it applies; LEGKILO_GRIDSCAN / lk_stream_grid
    bool resident_enable = true;  // scans of small buckets as one resident launch (lk_scan_stream_kernel); LEGKILO_RESIDENT=0 / lk_stream_resident(h, 0): per-bucket launches
    bool spec_enable = false;     // LEGKILO_SPEC=1 / lk_stream_pipeline(h, 1); measured slower than the sequential order: off by default
    LkFilter* d_snap = nullptr;   // 2 posterior snapshots (dev_snapshot_posterior)
    struct ScanResult {            // what a stream-path scan hands back: written by ONE kernel into host-mapped pinned memory (no copies, one sync)
        lk_pose pose;
        unsigned int ctr[LK_CTR_COUNT];
        int resume[4];               // scan-resident kernel: LkResume's bf, bi, fb_bucket (where the launch stopped), 0
        unsigned int seq, pad_;      // written last: the host may poll it instead of blocking in hipStreamSynchronize
    };
    uint64_t resident_scans = 0, resident_relaunches = 0, grid_scans = 0, grid_relaunches = 0;   // lk_stream_resident_stats
    unsigned int test_stall_ms = 0;   // lk_test_stall: the next resident launches run with this bound and an injected stall (error-path test)
    unsigned int result_seq = 0;
    ScanResult* h_result = nullptr;   // hipHostMalloc(mapped)
    ScanResult* d_result = nullptr;   // its device-side address
    LkFilter* d_fbackup = nullptr;   // filters[0] as it was when the running scan started: what an LK_ERR_TIMEOUT puts back (grid-resident and pipelined paths)
    bool fbackup_valid = false;
    int2* d_ids = nullptr;        // [max_scan] root codes of the speculative residual pass
    uint64_t spec_buckets = 0, spec_tiles = 0, spec_redo_total = 0, res_redo_total = 0;
    unsigned int spec_redo_seen = 0, res_redo_seen = 0;
    double acc_norm = 1.0;
    bool q_diag = true;        // d_Q holds a diagonal matrix (zero-initialised; lk_set_Q re-checks)
    // frozen-map grid of batch replay (LkMap::grid): valid until the map changes
    LkMap fmap = {};           // h->map + the grid fields; h->map itself always has grid_on = 0 (the streaming path mutates the map)
    size_t grid_cap = 0;       // grid cells allocated behind the max_nodes match records of map.match
    bool grid_valid = false;   // the grid describes the current map
    uint64_t map_gen = 0;      // counts the map snapshots batch replays have frozen: frozen_map() bumps it whenever the map had changed since the last one
    uint64_t ov_gen = 0;       // the snapshot the last overlay replay ran against (lk_overlay_export reads base blocks / planes of THAT map)
    bool grid_enable = true;   // LEGKILO_GRID=0 keeps batch replay on the hash table (A/B)
    int* d_grid_mm = nullptr;
    DevBuf pre;                   // scratch of the lidar front end: lk_decode_scan(_dev), lk_preprocess_scan(_dev), lk_decode_scans_dev, lk_process_raw_scan (FrontPool)
    DevBuf mcl;                   // scratch of lk_downsample_clouds(_dev) (MclPool)
    // batch replay with a per-scan insert overlay (lk_overlay_kernels.h): the pools of all slots, grow-only
    LkOverlay ov = {};
    uint32_t ov_slots = 0;                                // slots the pools were allocated for
    uint32_t ov_want_roots = 0, ov_want_nodes = 0, ov_want_blocks = 0;   // lk_overlay_reserve (0: derived from the scan size)
    uint32_t ov_last_slots = 0;                           // slots of the last overlay replay (lk_overlay_export / lk_overlay_stats)
    uint32_t ov_hw_roots = 0, ov_hw_nodes = 0, ov_hw_blocks = 0;   // high-water marks of the last replay (any slot): the next replay's pools are sized from them
    size_t ov_hw_npts = 0;                                // ... which belong to scans of this size
    bool ov_runs = false, ov_hw_runs = false;             // the overlay replay at hand replays runs of scans (a slot's size is its run's point total); ... and so did the one the marks are from
    size_t ov_pool_bytes = 0;                             // bytes the overlay pools hold (lk_overlay_pool_bytes)
    DevBuf ov_priors;                                     // LkFilter[S]: the batch's priors, kept for the retry after a pool overflow
    DevBuf query;                                         // lk_match_points: inputs + outputs of a query
    DevBuf ov_res;                                        // scan-resident recorded-run replay with insert: [S] next bucket, [S] bucket with fallback items, stopped-scan counter
    unsigned int ov_res_rounds = 0;                       // launches of the scan-resident kernel in the last such replay
    DevBuf bucket_tab;                                    // lk_bucket_pose[flat buckets] of the last _cloud run replay (lk_runs_bucket_poses)
    size_t bucket_n = 0;                                  // its records; 0: the handle's last batch replay recorded nothing
    unsigned int* d_ov_status = nullptr;
    // input order of device-resident batches (lk_batch_order): the batches the frozen-map batch entries have seen, with the library's voxel-ordered copy
    struct OrdEntry {
        const lk_point* src = nullptr;     // the caller's buffer and the shape it was seen with
        size_t n_scans = 0, n_pts = 0, n_buckets = 0;
        uint64_t off_hash = 0;
        bool as_given = false;             // the batch already was in voxel order: replayed where it lies, no copy, no stamp
        lk_point* copy = nullptr;          // voxel-ordered copy (every bucket of every scan sorted by root-voxel key under the priors of the first sight)
        size_t copy_bytes = 0;
        unsigned long long* d_ref = nullptr;   // device, LK_ORDW_COUNT words (lk_batch_stamp.h): the stamp the copy was made from, the stamp of the replay before, a decision pair per ring stream
        bool have_copy = false;            // the copy holds the buffer's content as of the last sort (as far as the host knows: h_seen says what the device found)
        unsigned int* h_seen = nullptr;    // host-mapped, written by the device: replays in a row that found the same content stamp; LK_ORD_SORTED while the copy is current
        unsigned int* d_seen = nullptr;
        unsigned int probes = 0;           // counting replays enqueued for the content at hand (h_seen may not show them yet)
        bool waited = false;               // ... and the replays in flight have been waited for once, when h_seen lagged behind that number
        uint64_t tick = 0;
    };
    OrdEntry ord[2];
    uint64_t ord_tick = 0, ord_examined = 0, ord_sorted = 0, ord_stale = 0;
    int batch_order_mode = 1;              // LK_BATCH_ORDER_AUTO; LEGKILO_BATCH_ORDER=0 / lk_batch_order(h, 0): replay every batch as given
    int batch_order_after = 2;             // a batch is sorted once this many replays in a row have found the same content in its buffer (the sort pays for itself after ~10)
    // leg kinematics front end (lk_kin.hip): configuration, the state carried from message to message, scratch
    bool kin_configured = false;
    lk_kin_config kin_cfg = {};
    lk_kin_frontend_state kin_fe = {};
    DevBuf kin;                   // keep flags, ranks, transition maps, their scan, status words; the scan split's tables (either record kind)
    // IMU front end (lk_kin.hip): the redundancy flag, the state carried from message to message, scratch
    bool imu_configured = false, imu_redundancy = false;
    lk_imu_frontend_state imu_fe = {};
    DevBuf imu;                   // message offsets, keep flags, ranks, status words
    DevBuf ff;                    // lk_first_frame(_dev): world / body clouds, acc_norm
    bool profiling = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::map<std::string, ProfEntry> prof;
    std::string err;
    DevBuf traj;                  // lk_traj_ate_dev / lk_runs_ate_dev and the _rpe_ pair (lk_traj.hip): offset tables, partner words, the records, the refusal word
    DevBuf c2c;                   // lk_clouds_c2c(_dev), lk_clouds_mme(_dev), lk_clouds_align(_dev), lk_clouds_transform_dev (lk_c2c.hip): tables, bounds, grids, keys and sorted records of the indexed clouds, per-point arrays, the records, an alignment's T0 / records / done words
    DevBuf c2c_io;                // lk_clouds_c2c, lk_clouds_mme, lk_clouds_align: device copies of the host clouds and of the host per-point arrays
};

extern thread_local std::string g_err;   // defined in legkilo_hip.hip (lk_last_error(NULL) reads it)

static int fail(lk_handle* h, int code, const std::string& msg) {
    g_err = msg;
    if (h) h->err = msg;
    return code;
}
#define HIPCHK(h, call)                                                                               \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(h, LK_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));            \
    } while (0)

#define LKCHK(call)                        \
    do {                                   \
        const int rc_ = (call);            \
        if (rc_ != LK_OK) return rc_;      \
    } while (0)

template <typename F>
static int launch(lk_handle* h, const char* name, F&& f) {
    if (h->profiling) {
        HIPCHK(h, hipEventRecord(h->ev0, h->stream));
        f();
        HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        HIPCHK(h, hipEventSynchronize(h->ev1));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        ProfEntry& p = h->prof[name];
        p.launches += 1;
        p.total_ms += ms;
    } else {
        // LEGKILO_TRACE_LAUNCH=<prefix> (debug aid): every launch whose name starts with the prefix is announced on stderr and waited for -
        // the last name printed before a "Memory access fault by GPU" is the kernel that made it
        static const char* trace = getenv("LEGKILO_TRACE_LAUNCH");
        const bool tr = trace && strncmp(name, trace, strlen(trace)) == 0;
        if (tr) fprintf(stderr, "[launch] %s\n", name), fflush(stderr);
        f();
        if (tr) HIPCHK(h, hipDeviceSynchronize());
    }
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}
#define LAUNCH(h, name, ...)                                   \
    do {                                                       \
        int rc_ = launch(h, name, [&]() { __VA_ARGS__; });     \
        if (rc_ != LK_OK) return rc_;                          \
    } while (0)

// Every device allocation of this library.  LEGKILO_POISON_POOLS=1 (test aid): the fresh memory is filled with 0x5a bytes instead of whatever the
// allocator hands out - in a young process zeros, in a long-lived one somebody's old data - so that a kernel which trusts memory nobody has
// written meets garbage in EVERY run (the whole GPU suite is run that way once per round: tools/gpu_poison_suite.sh)
// (set when the process starts, or by a test around single calls: both count)
static bool lk_poison_pools() {
    static const bool at_start = getenv("LEGKILO_POISON_POOLS") != nullptr;
    return at_start || getenv("LEGKILO_POISON_POOLS") != nullptr;
}
static hipError_t lk_hip_malloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && lk_poison_pools() && bytes) {
        e = hipMemset(*p, 0x5a, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();   // (the fill runs on the null stream, the library's streams do not wait for that one)
    }
    return e;
}
template <typename T>
static hipError_t lk_hip_malloc(T** p, size_t bytes) {
    return lk_hip_malloc(reinterpret_cast<void**>(p), bytes);
}
#define hipMalloc(p, n) lk_hip_malloc((p), (n))

// A fixed pool of the handle (allocated once, freed by lk_destroy).  LkMap and its like go to kernels by value and stay plain structs:
// only the host remembers what it handed out.
template <typename T>
static hipError_t pool_alloc(lk_handle* h, T** out, size_t bytes) {
    const hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess) h->pools.push_back(*out);
    return e;
}

static void buf_release(DevBuf& b) {
    if (b.p) b.pinned ? hipHostFree(b.p) : hipFree(b.p);
    b.p = nullptr, b.cap = 0;
}
// Room for `bytes` in a grow-only buffer.  Large enough already: nothing happens (no synchronisation, no HIP call).  Otherwise the handle's
// stream is waited for - every user of these buffers runs there - and the buffer is replaced by one of bytes + slack; an allocation that
// fails leaves it empty, so the next call behaves like a first call.
static int reserve(lk_handle* h, DevBuf& b, size_t bytes, size_t slack = 0) {
    if (bytes <= b.cap) return LK_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    buf_release(b);
    if (!b.listed) h->grown.push_back(&b), b.listed = true;
    HIPCHK(h, b.pinned ? hipHostMalloc(&b.p, bytes + slack, hipHostMallocDefault) : hipMalloc(&b.p, bytes + slack));
    b.cap = bytes + slack;
    return LK_OK;
}
// The ragged tables' device copy and its pinned staging twin.  The synchronisation is unconditional and not about growth: a previous
// call's upload out of the staging buffer must have finished before the host overwrites it.
static int rag_reserve(lk_handle* h, size_t bytes) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    LKCHK(reserve(h, h->rag, bytes, bytes / 2));
    return reserve(h, h->rag_stage, bytes, bytes / 2);
}

// device temporaries of one call: freed on every return path
struct DevTemps {
    std::vector<void*> ptrs;
    ~DevTemps() {
        for (void* p : ptrs)
            if (p) hipFree(p);
    }
    template <typename T>
    hipError_t alloc(T** out, size_t bytes) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) ptrs.push_back(p);
        *out = (T*)p;
        return e;
    }
};

// The pool compaction of lk_map_slide / lk_map_clear_outside (lk_map_kernels.h), in steps, so that lk_overlay_commit (overlay unit) can put its own
// between them: begin - the map's counters, the flag and rank arrays, zeroed; x_* > 0: room for the records of a second pool (a slot's overlay)
// flagged BEHIND the map's, so that one scan ranks the survivors first and those records behind them; mark - lk_slide_mark_kernel (box, and `drop`
// if asked for); count - the exclusive scans and their totals, nothing of the map written so far; move - survivors to their ranks, the root table
// cleared, the kept roots renumbered; finish - the table rebuilt from kept[0 .. n_roots), the counters set, the error word read.  The functions are
// the main unit's.
struct MapCompact {
    DevTemps tmp;                                                // freed on every exit path
    unsigned int n_nodes = 0, n_blocks = 0, n_roots = 0;         // the map's counters at begin()
    unsigned int x_nodes = 0, x_blocks = 0, x_roots = 0;         // the second pool's records
    unsigned int *alive_node = nullptr, *alive_block = nullptr;  // [n_nodes + x_nodes], [n_blocks + x_blocks]
    unsigned int *new_node = nullptr, *new_block = nullptr;      // their exclusive scans
    unsigned int *drop = nullptr;                                // [n_nodes]: roots to remove whatever the box says
    unsigned int *cnt = nullptr;                                 // [4]: kept, removed, two words of the caller's
    lk_root_rec* kept = nullptr;                                 // [n_roots + x_roots]
    unsigned int kept_roots = 0, removed_roots = 0;              // mark()
    unsigned int live_nodes = 0, live_blocks = 0;                // count(): the map's survivors ...
    unsigned int all_nodes = 0, all_blocks = 0;                  // ... and with the second pool's flagged records
};

// LEGKILO_XID=0: the generic residual kernels instead of those specialised for ext_R == I (the tests' reference); read once per process
static bool lk_xid_enabled() {
    static const bool v = getenv("LEGKILO_XID") == nullptr || atoi(getenv("LEGKILO_XID")) != 0;
    return v;
}

// Rows of a bounds launch over many clouds (grid = clouds x rows, the rows of a cloud stride over its points): a row per 4096 points of the
// biggest cloud, at most 1024, and at most 2^18 blocks in all   (map clouds: a cloud per file; cloud scores)
static inline unsigned int bounds_rows(size_t clouds, size_t biggest) {
    return (unsigned int)std::min<size_t>(std::min<size_t>(1024, std::max<size_t>(1, (1u << 18) / clouds)), std::max<size_t>(1, biggest / 4096));
}

static unsigned int next_pow2(unsigned int v) {
    unsigned int p = 1;
    while (p < v) p <<= 1;
    return p;
}

static int check_map_errors(lk_handle* h, const unsigned int* fetched = nullptr) {
    unsigned int ctr[LK_CTR_COUNT];
    if (fetched) {
        memcpy(ctr, fetched, sizeof(ctr));
    } else {
        HIPCHK(h, hipMemcpyAsync(ctr, h->map.counters, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (ctr[LK_CTR_ERR] & LK_E_SPEC_TIMEOUT) {
        // not sticky: the word is cleared, so the handle stays usable once its map has been restored
        const unsigned int rest = ctr[LK_CTR_ERR] & ~LK_E_SPEC_TIMEOUT;
        HIPCHK(h, hipMemcpyAsync(h->map.counters + LK_CTR_ERR, &rest, sizeof(rest), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        // the filter keeps its PRE-SCAN state on every path: the resident kernels' and the pipelined launches' scans start with a copy of
        // filters[0] that is put back here (a scan-resident launch given up returns before its write-back, but a scan picked up again after
        // fallback items has written the filter once)
        if (h->fbackup_valid) {
            HIPCHK(h, hipMemcpyAsync(h->d_filters, h->d_fbackup, sizeof(LkFilter), hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        h->fbackup_valid = false;
        return fail(h, LK_ERR_TIMEOUT, "a bounded device-side wait of the stream path timed out (device fault, or a pre-empted / debugged GPU; "
                                       "LEGKILO_RESIDENT_TIMEOUT_MS raises the bound): the filter keeps its state from before the scan, the map may hold a partial "
                                       "insert - restore it (lk_map_import) and replay the scan");
    }
    h->fbackup_valid = false;
    if (ctr[LK_CTR_ERR]) {
        char buf[160];
        snprintf(buf, sizeof(buf), "device pool overflow (bits 0x%x: 1 hash, 2 nodes, 4 point blocks, 8 scratch, 16 bad blob)", ctr[LK_CTR_ERR]);
        return fail(h, LK_ERR_CAPACITY, buf);
    }
    return LK_OK;
}


#define LK_SCAN_WAVE_MAX 512   // largest bucket of the one-wave-per-scan chains (dev_scan_wave, lk_rag_ov_front_kernel): up to eight tiles, added in tile order
extern "C" int spec_join(lk_handle* h);   // main unit: joins the pipelined stream path's insert stream
#define CHECK_H(h)                                                         \
    do {                                                                   \
        if (!(h)) return fail(nullptr, LK_ERR_INVALID, "null handle");     \
        hipSetDevice((h)->cfg.device_id);                                  \
        if ((h)->spec_open) {                                              \
            int rcj_ = spec_join(h);                                       \
            if (rcj_ != LK_OK) return rcj_;                                \
        }                                                                  \
    } while (0)
#define CHECK_SLOT(h, s)                                                                  \
    do {                                                                                  \
        if ((s) >= (h)->cfg.n_slots) return fail(h, LK_ERR_INVALID, "slot out of range"); \
    } while (0)

#define LK_CTR_GRID_XCC 15   // LkMap.counters[15]: XCC ids (one bit each) the working blocks of the last one-XCD launch of the grid-resident stream kernel ran on
static inline void imu_noise(const lk_config& c, double* Rn) {   // diag of R of an IMU observation (KILO.cc:251-253)
    Rn[0] = Rn[1] = c.imu_acc_meas_noise;
    Rn[2] = c.imu_acc_z_meas_noise;
    Rn[3] = Rn[4] = Rn[5] = c.imu_gyr_meas_noise;
}

// The message records between a scan's buckets, under the values of the public msg_kind arguments; the size of one record (MSG_NONE: tables
// without messages are laid out with lk_imu's stride, which nothing reads).
enum MsgKind { MSG_NONE = 0, MSG_IMU = 1, MSG_KIN = 2 };
static inline size_t msg_record_bytes(int kind) { return kind == MSG_KIN ? sizeof(lk_kin_imu) : sizeof(lk_imu); }
// What an LkRagged takes from the handle, whatever built its tables: the message stride, the measurement noises, the gravity scale, Q's shape.
static inline void rag_from_handle(const lk_handle* h, int msg_kind, LkRagged* rg) {
    rg->msg_stride = (int)(msg_record_bytes(msg_kind) / sizeof(double));
    rg->kin_noise = h->cfg.kin_meas_noise;
    rg->q_diag = h->q_diag ? 1 : 0;
    rg->acc_scale = h->cfg.gravity / h->acc_norm;
    imu_noise(h->cfg, rg->Rn);
}

// Tables of a live run (lk_run_scans_dev), built once per call on the device by run_tables() in h->ragdev: the CSR bucket tables of all its scans
// (BucketTables in the main unit, offsets counted from the run's first point) and, per scan, what a resident stream kernel wants besides them.  The host gets the scans' first buckets and lk_rag_scan_summary_kernel's summaries: a few words per scan, read back once.
struct RunTables {
    const unsigned long long* d_ps = nullptr;   // first point of every bucket of the run (+ the end)
    const double* d_tb = nullptr;               // its time
    const unsigned int* d_nbp = nullptr;        // [S][2] { buckets, 0 }
    const unsigned int* d_mo = nullptr;         // [S + 1] prefix sum of the scans' message counts (null: no messages)
    unsigned int* d_sync = nullptr;             // [S][4] the grid-resident kernel's barrier words, zeroed
    int* d_resume = nullptr;                    // [S] LkResume, reset
    std::vector<unsigned int> bstart;           // [S + 1] first bucket of every scan
    std::vector<unsigned int> sum;              // [S][4] buckets, largest bucket, smallest bucket, first message
    unsigned int first_unsorted = 0xffffffffu;  // first scan whose curvature decreases or is not finite
};

// ---- shared between the translation units (all with C linkage: they are defined inside the units' extern "C" regions)
extern "C" {
// main unit (legkilo_hip.hip)
int frozen_map(lk_handle* h, LkMap* out);                    // the handle's map + the frozen-map grid of the batch replays (rebuilt when the map has changed)
int join_side_streams(lk_handle* h);
int zero_scan_counters(lk_handle* h, uint32_t first_slot, uint32_t n_slots);
int fetch_poses(lk_handle* h, lk_pose* out, int n);
int export_map_blob(lk_handle* h, const LkMap& m, unsigned int hash_cap, void* blob, size_t* bytes);
int replay_scans(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin, int msg_kind,
                 const uint32_t* n_msg, const void* msgs, bool msgs_on_device, lk_pose* out);   // lk_batch_replay_scans(_kin / _imu)_dev
int ragged_replay(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const uint32_t* n_buckets, const uint32_t* bucket_off,
                  const double* bucket_dt, const double* t_begin, const uint32_t* n_imu, const void* imus, int msg_kind, lk_pose* out, bool with_insert = false);
int run_tables(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const double* t_begin, const uint32_t* n_msg, struct RunTables* out);
__global__ void lk_set_times_kernel(LkFilter* filters, int n, double t);
__global__ void __launch_bounds__(LK_WAVE, 2) lk_rag_advance_kernel(LkFilter* filters, const double* __restrict__ Q, LkRagged rg, int b, int msg_kind);
int upload_xyz_as_points(lk_handle* h, const float* xyz, size_t n);   // n x 3 floats -> h->d_scan as lk_point records
int compact_begin(lk_handle* h, MapCompact* mc, unsigned int x_nodes, unsigned int x_blocks, unsigned int x_roots);
int compact_mark(lk_handle* h, MapCompact* mc, const LkSlideBox& box, bool with_drop);
int compact_count(lk_handle* h, MapCompact* mc);
int compact_move(lk_handle* h, MapCompact* mc);
int compact_finish(lk_handle* h, MapCompact* mc, unsigned int n_nodes, unsigned int n_blocks, unsigned int n_roots, bool validate_ids);
// stream unit (lk_stream.hip)
int run_scan(lk_handle* h, const lk_point* pts, const lk_point* d_pts, size_t n, double t_begin, const lk_imu* imus, size_t n_imu, const lk_kin_imu* kins,
             size_t n_kin, float* xyz_world_out, lk_pose* out);          // the bucket loop of KILO::process on a sorted cloud that is in HBM (and on the host, for the bucket bounds)
// overlay unit (lk_overlay.hip)
void ov_free(lk_handle* h);
// lk_ovscan.hip (LK_TU_OVSCAN: the scan-resident kernel of the recorded-run replay with insert, a unit of its own for the build time): one launch of it
int ov_scan_launch(lk_handle* h, bool xid, int S, hipStream_t st, const LkMap& fmap, const LkOverlay& ov, LkFilter* fl, const LkRagged& rg, const lk_point* d_pts, int msg_kind,
                   int* cur, int* fb_b, unsigned int* pending);
// lk_ovrun.hip (LK_TU_OVSCAN as well: lk_ovscan.hip compiled once more for its run-resident instantiations - lk_batch_replay_overlay_runs_dev)
int ov_run_launch(lk_handle* h, bool xid, int S, hipStream_t st, const LkMap& fmap, const LkOverlay& ov, LkFilter* fl, const LkRagged& rg, const lk_point* d_pts, int msg_kind,
                  int* cur, int* fb_b, unsigned int* pending);
int overlay_ragged_launch(lk_handle* h, const lk_point* d_pts, size_t S, const LkRagged& rg, const double* d_tbegin, int biggest, size_t ldb, const int* max_n,
                          size_t max_scan_pts, int msg_kind, lk_pose* out, size_t n_poses = 0);
}

// The tail of a synchronous batch entry: the poses if the caller wants them (fetch_poses synchronises), else only the wait.
static inline int fetch_poses_or_sync(lk_handle* h, lk_pose* out, int n) {
    if (out) return fetch_poses(h, out, n);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

// The non-empty buckets of a uniform batch (the empty ones are skipped by every entry), none above max_scan_points; *biggest: the largest of them.
// entry_check(b): what the calling entry asks of every bucket, empty ones included, before this bucket's size is looked at.
template <class Check>
static inline int live_buckets(lk_handle* h, const uint32_t* bucket_off, size_t n_buckets, std::vector<size_t>& live, size_t* biggest, Check&& entry_check) {
    for (size_t b = 0; b < n_buckets; ++b) {
        LKCHK(entry_check(b));
        if (bucket_off[b + 1] <= bucket_off[b]) continue;
        const size_t nb = (size_t)(bucket_off[b + 1] - bucket_off[b]);
        if (nb > h->map.max_scan) return fail(h, LK_ERR_CAPACITY, "bucket exceeds max_scan_points");
        if (biggest) *biggest = std::max(*biggest, nb);
        live.push_back(b);
    }
    return LK_OK;
}
static inline int live_buckets(lk_handle* h, const uint32_t* bucket_off, size_t n_buckets, std::vector<size_t>& live) {
    return live_buckets(h, bucket_off, n_buckets, live, nullptr, [](size_t) { return LK_OK; });
}

// Slot groups of a synchronous batch replay: the batch's slots cut into `n` ranges, range g on stream g (the handle's own, then side[]).  The scans are
// independent, so the groups touch disjoint filters, partials and pools and only read the map.  Profiling mode (per-launch events + sync on the
// handle's stream) and small batches stay on one stream:
//   frozen map: h->replay_groups groups (3: measured best of 1..8; LEGKILO_REPLAY_GROUPS) from kReplayGroupSlots slots per group on;
//   overlay:    kOverlayGroups from kOverlayGroupSlots slots per group on.
// fork() makes the side streams wait for what the handle's stream holds so far (if it fails, nothing of this call is on a side stream yet and the
// entry just returns), join(rc) takes what the enqueue in between returned: on success the handle's stream waits for every group; on failure every
// stream is waited for HERE - a failed launch must not leave the side streams writing filters, partials and pools behind the caller's back.
// Nothing a caller can observe says whether a batch was split: tests/test_gpu_parity.py (OV_GROUPS, OV_GROUP_SLOTS of test_batch_replay_overlay[groups];
// S = 6 / 7 of test_batch_replay_frozen_map) and tests/test_dev_bounds.py size their batches by these values - change them together.
constexpr int kReplayGroupSlots = 2, kOverlayGroups = 4, kOverlayGroupSlots = 64;
static_assert(kOverlayGroups <= lk_handle::kMaxGroups, "a stream per group");
struct SlotGroups {
    lk_handle* h;
    int S, n;
    hipStream_t stream[lk_handle::kMaxGroups];
    SlotGroups(lk_handle* h_, int S_, int groups, int min_slots_per_group) : h(h_), S(S_), n((!h_->profiling && S_ >= min_slots_per_group * groups) ? groups : 1) {
        stream[0] = h->stream;
        for (int g = 1; g < lk_handle::kMaxGroups; ++g) stream[g] = h->side[g - 1];
    }
    int first(int g) const { return (int)((long)S * g / n); }
    int count(int g) const { return first(g + 1) - first(g); }
    int fork() const {
        if (n > 1) HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
        for (int g = 1; g < n; ++g) HIPCHK(h, hipStreamWaitEvent(stream[g], h->ev_fork, 0));
        return LK_OK;
    }
    int join(int rc) const {
        if (rc == LK_OK) rc = wait_for_groups();
        if (rc != LK_OK)
            for (int g = 0; g < n; ++g) (void)hipStreamSynchronize(stream[g]);   // error path: nothing of this call keeps running
        return rc;
    }
    int wait_for_groups() const {   // everything after this point on h->stream sees every group's results
        for (int g = 1; g < n; ++g) {
            HIPCHK(h, hipEventRecord(h->ev_join[g - 1], stream[g]));
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join[g - 1], 0));
        }
        return LK_OK;
    }
};
