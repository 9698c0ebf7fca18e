// lk_overlay.hip - the overlay translation unit of liblegkilo_hip.so (see lk_internal.h): batch replay WITH the map insert - every scan on its own
// copy-on-write overlay of the handle's map (lk_overlay_kernels.h) - and the entry points that launch it.
#define LK_TU_OVERLAY 1
#include "lk_internal.h"

// Round 6: the FRONT of a bucket index of the ragged batch with insert as ONE launch when every bucket holds <= LK_SCAN_WAVE_MAX points (a recorded
// scan's 2 ms bins): lk_rag_advance_kernel (messages + predict), lk_ov_residual_kernel, lk_update_wave_ragged_kernel, lk_ov_begin_kernel and
// lk_ov_reproject_kernel were five one-wave-per-scan launches, each paying a launch boundary (~5 us for 1 024 one-wave workgroups whatever they do) and
// its own load / store of the filter's 7.6 KB.  Here one wave per scan runs the five bodies back to back - the one-wave filter cores and the tile code
// of dev_scan_wave, the overlay lookup of lk_ov_residual_kernel - with state and covariance in LDS from the first message to the update.  Same device
// functions, same order of sums (tile totals in tile order, as lk_update_wave_kernel adds up to eight of them): bit-identical to the five launches
// (test_batch_replay_overlay_ragged compares both against the oracle).
extern "C++" {
template <bool XID>
__global__ void __launch_bounds__(LK_WAVE, 2)
    lk_rag_ov_front_kernel(LkMap base, LkOverlay ov, LkParams pr, LkFilter* filters, const double* __restrict__ Q, LkRagged rg, const lk_point* __restrict__ d_pts,
                           int b, int msg_kind) {
    __shared__ WaveSmem sm;
    __shared__ double rows[64 * LK_ROW2];
    const int slot = blockIdx.x, lane = threadIdx.x;
    const LkMap pm = ov_slot_map(ov, (unsigned int)slot);
    if (b >= rag_nb(rg, slot)) {   // this scan has run out of buckets: the passes behind this one must find its work lists empty (lk_ov_begin_kernel ran for every slot)
        dev_bucket_begin_wave(pm);
        return;
    }
    LkFilter* f = &filters[slot];
    const double* T = rag_t(rg, slot);
    for (int e = lane; e < 900; e += LK_WAVE) sm.P[e] = f->P[e];
    if (lane < 36) sm.x[lane] = f->x[lane];
    double t_upd = f->last_update_t, t_pred = f->last_predict_t;
    __syncthreads();
    const double tb = T[b];
    const LkRagBucket rb = rag_bucket(rg, slot, b, msg_kind != 0);   // (runs: the messages and the look-back are the owning scan's)
    if (msg_kind) {   // lk_rag_advance_kernel: the scan's messages stamped before this bucket that no earlier bucket has consumed (KILO.cc:379-390)
        const size_t mstride = msg_kind == 2 ? 33 : 7;
        const unsigned int q0 = rb.q0, q1 = rb.q1;
        for (unsigned int q = q0; q < q1; ++q) {
            const double* m = rg.imu + mstride * (size_t)q;
            const double tm = m[0];
            if (!(tm < tb)) break;
            if (!rb.first && tm < T[b - 1]) continue;
            wave_predict_core(sm, Q, tm - t_upd, tm - t_pred, lane, rg.q_diag != 0);
            t_pred = tm;
            if (msg_kind == 2) wave_kin_update_core(sm, rows, m, rg.acc_scale, rg.Rn, rg.kin_noise, lane);
            else wave_imu_update_core(sm, m + 1, m + 4, rg.acc_scale, rg.Rn, lane);
            t_upd = tm;
        }
    }
    wave_predict_core(sm, Q, tb - t_upd, tb - t_pred, lane, rg.q_diag != 0);   // KILO.cc:111-115
    t_pred = tb;
    // lk_ov_residual_kernel: the bucket's tiles against base map + the scan's overlay, under the predicted state in LDS
    const unsigned long long* po = rag_pt_off(rg, slot);
    const lk_point* pts = d_pts + po[b];
    const int n = (int)(po[b + 1] - po[b]);
    BucketConst bc;
#pragma unroll
    for (int i = 0; i < 9; ++i) bc.R[i] = sm.x[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) bc.p[i] = sm.x[9 + i];
    {
        const double* P = sm.P;
        bc.Prr = S3{P[0], P[1], P[2], P[31], P[32], P[62]};
        bc.Ppp = S3{P[3 * 30 + 3], P[3 * 30 + 4], P[3 * 30 + 5], P[4 * 30 + 4], P[4 * 30 + 5], P[5 * 30 + 5]};
    }
    LkOvView ovv;
    ovv.keys = ov.keys + (size_t)slot * ov.hash_cap;
    ovv.hash_mask = ov.hash_cap - 1;
    ovv.match = ov.match + (size_t)slot * ov.nodes_cap;
    ovv.nodes = ov.nodes + (size_t)slot * ov.nodes_cap;
    ovv.bits = ov.bits + (size_t)slot * ov.bit_words;
    ResidualOut ro;
    ro.h6 = nullptr, ro.z = nullptr, ro.R = nullptr, ro.valid = nullptr, ro.world = nullptr, ro.ids = nullptr;
    double totv = 0.0;   // tot[j] in lanes 0..31
    for (int i0 = 0; i0 < n; i0 += LK_WAVE) {
        __builtin_amdgcn_wave_barrier();   // the previous tile's reads of the rows are complete
        const double a = residual_tile<false, 3, XID, true, false>(base, pr, bc, reinterpret_cast<const float4*>(pts), i0 + lane, n, rows, lane, ro, (size_t)0, &ovv);
        totv += (lane < 29) ? a : 0.0;
    }
    // lk_update_wave_ragged_kernel (update_only): the posterior the insert reads
    const int N = (int)(lane_bcast<28>(totv) + 0.5);
    if (lane == 0) {
        if (rg.run_scan && rb.first) f->n_buckets = 0u, f->n_updates = 0u, f->n_effect = 0ull;   // runs: the counters are the scan's own
        f->last_predict_t = t_pred;
        f->n_buckets += 1;
        f->last_N = N;
        f->updated = N > 0;
        if (N > 0) {
            f->n_updates += 1;
            f->n_effect += (unsigned long long)N;
        }
        f->last_update_t = N > 0 ? tb : t_upd;   // KILO.cc:212
    }
    if (N > 0) wave_update_core(sm, totv, N, lane);
    __syncthreads();
    for (int e = lane; e < 900; e += LK_WAVE) f->P[e] = sm.P[e];
    if (lane < 36) f->x[lane] = sm.x[lane];
    if (rb.pose) rag_write_pose(rb.pose, sm.x, f, lane);   // runs: the scan's last bucket
    // the re-projection below reads the posterior through the filter record, like every other kernel of the insert - written by THIS wave: its stores
    // have to be acknowledged before its loads go out (workgroup scope = s_waitcnt; an agent-scope fence here is an L2 write-back + invalidate per
    // wave, 1 024 of them per launch: the first version of this kernel was 6 ms SLOWER than the five launches for it)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    // lk_ov_begin_kernel, lk_ov_reproject_kernel
    dev_bucket_begin_wave(pm);
    for (int i = lane; i < n; i += LK_WAVE) {
        const int r = ov_reproject_point(base, ov, pr, filters, pts, i, (unsigned int)slot);
        ov.ptroot[(size_t)slot * ov.scan_cap + i] = r;   // for lk_ov_point_geom_kernel
    }
}

// Runs, buckets above LK_SCAN_WAVE_MAX points (the update is lk_update_wave_ragged_kernel's, which knows no scans): the pose of every scan whose last bucket
// is bucket b of its run, from the posterior that update has just written.
__global__ void __launch_bounds__(LK_WAVE) lk_rag_pose_tap_kernel(const LkFilter* __restrict__ filters, LkRagged rg, int b) {
    const int slot = blockIdx.x;
    if (b >= rag_nb(rg, slot)) return;
    const LkRagBucket rb = rag_bucket(rg, slot, b, false);
    if (rb.pose) rag_write_pose(rb.pose, filters[slot].x, &filters[slot], (int)threadIdx.x);
}
// Runs launch by launch, small buckets and large (the _cloud entries only): the record of bucket b of every run that has one, from the filter record
// as the update (lk_rag_ov_front_kernel's, lk_update_wave_ragged_kernel's) has just left it - the insert behind it reads that record and changes none of it.
__global__ void __launch_bounds__(LK_WAVE) lk_rag_bucket_tap_kernel(const LkFilter* __restrict__ filters, LkRagged rg, int b) {
    const int slot = blockIdx.x;
    if (!(rg.run_scan && rg.bucket_pose) || b >= rag_nb(rg, slot)) return;
    const LkFilter* f = &filters[slot];
    const unsigned long long* po = rag_pt_off(rg, slot);
    rag_write_bucket(rg.bucket_pose + rg.bstart[slot] + (unsigned int)b, f->x, rag_t(rg, slot)[b], po[b], (unsigned int)(po[b + 1] - po[b]), (unsigned int)f->last_N,
                     (int)threadIdx.x);
}
}   // extern "C++"

extern "C" {

// What lk_overlay_export and lk_overlay_commit ask before they read an overlay: the pools of a replay are there, and the handle's map still is the
// one that replay ran against.
static int ov_readable(lk_handle* h, const char* verb) {
    if (!h->ov.counters || !h->ov_last_slots) return fail(h, LK_ERR_STATE, "no overlay replay's pools are held by this handle (none has run, or lk_overlay_reserve released them)");
    // an overlay is not self-contained: split leaves keep their first points in the BASE map's blocks, lazily copied voxels their plane in the base
    // map's plane records.  Once the handle's map has changed (lk_process_scan, lk_map_update, lk_map_slide, lk_map_import, lk_overlay_commit, ...)
    // those ids may name other voxels: refuse instead of reading them
    if (!h->grid_valid || h->ov_gen != h->map_gen)
        return fail(h, LK_ERR_STATE, std::string("the handle's map has changed since the overlay replay: its overlays can no longer be ") + verb +
                                         " (export before the map is updated, slid or imported, or replay again)");
    return LK_OK;
}
// leaves the fast root pass left split (old points still in the handle's blocks) and lazily copied plane records are made whole
static int ov_make_whole(lk_handle* h, uint32_t slot) {
    hipLaunchKernelGGL(lk_ov_merge_split_kernel, dim3(64), dim3(LK_MB), 0, h->stream, h->map, h->ov, slot);
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}

int lk_overlay_export(lk_handle* h, uint32_t slot, void* blob, size_t* bytes) {
    CHECK_H(h);
    LKCHK(ov_readable(h, "exported"));
    if (slot >= h->ov_last_slots) return fail(h, LK_ERR_INVALID, "slot was not part of the last overlay replay");
    const LkOverlay& ov = h->ov;
    LKCHK(ov_make_whole(h, slot));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> keys(ov.hash_cap);
    HIPCHK(h, hipMemcpy(keys.data(), ov.keys + (size_t)slot * ov.hash_cap, sizeof(unsigned long long) * ov.hash_cap, hipMemcpyDeviceToHost));
    std::vector<int4> table(ov.hash_cap);
    for (unsigned int i = 0; i < ov.hash_cap; ++i) {
        if (keys[i] == LK_OV_EMPTY) {
            table[i] = make_int4(INT_MIN, INT_MIN, INT_MIN, LK_EMPTY);
        } else {
            int k3[3];
            ov_unpack_key(keys[i], k3);
            table[i] = make_int4(k3[0], k3[1], k3[2], (int)i);
        }
    }
    LkMap m = ov_slot_map(ov, slot);
    DevTemps tmp;
    HIPCHK(h, tmp.alloc(&m.hash, sizeof(int4) * ov.hash_cap));
    HIPCHK(h, hipMemcpy(m.hash, table.data(), sizeof(int4) * ov.hash_cap, hipMemcpyHostToDevice));
    return export_map_blob(h, m, ov.hash_cap, blob, bytes);
}

// Slot `slot`'s overlay becomes part of the handle's map, in HBM: the compaction of the map slide (MapCompact) with the base voxels the slot holds
// privately as the ones to remove, and the slot's private records ranked behind the survivors by the same scans.  Every refusal comes before
// compact_move, the first write to the map.
int lk_overlay_commit(lk_handle* h, uint32_t slot, uint32_t flags) {
    CHECK_H(h);
    LKCHK(ov_readable(h, "committed"));
    if (slot >= h->ov_last_slots) return fail(h, LK_ERR_INVALID, "slot was not part of the last overlay replay");
    if (flags & ~LK_COMMIT_ADOPT_FILTER) return fail(h, LK_ERR_INVALID, "unknown flag bits (LK_COMMIT_ADOPT_FILTER is the only flag)");
    LKCHK(join_side_streams(h));
    const LkOverlay& ov = h->ov;
    const LkMap pm = ov_slot_map(ov, slot);
    LKCHK(ov_make_whole(h, slot));
    unsigned int octr[LK_CTR_COUNT];
    HIPCHK(h, hipMemcpyAsync(octr, pm.counters, sizeof(octr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (octr[LK_CTR_ERR]) return fail(h, LK_ERR_STATE, "the slot's overlay carries an error word: the replay that made it was refused");
    const unsigned int pn = std::min(octr[LK_CTR_NODES], ov.nodes_cap), pb = std::min(octr[LK_CTR_BLOCKS], ov.blocks_cap);   // used ranges of the private pools (pn >= hash_cap: the root entries)
    if (pn < ov.hash_cap) return fail(h, LK_ERR_STATE, "the slot's node counter lies below its root entries");   // (the flag arrays are sized by it)
    MapCompact mc;
    LKCHK(compact_begin(h, &mc, pn, pb, ov.hash_cap));
    unsigned int* xa_node = mc.alive_node + mc.n_nodes;   // the private records' part of the flag and rank arrays
    unsigned int* xa_block = mc.alive_block + mc.n_blocks;
    const unsigned int* xn_node = mc.new_node + mc.n_nodes;
    const unsigned int* xn_block = mc.new_block + mc.n_blocks;
    const unsigned int root_grid = (ov.hash_cap + 255) / 256;
    LAUNCH(h, "ov_commit_mark", hipLaunchKernelGGL(lk_ov_commit_mark_kernel, dim3(root_grid), dim3(256), 0, h->stream, h->map, ov, slot, pn, pb, mc.drop, xa_node, xa_block, mc.cnt + 2));
    LKCHK(compact_mark(h, &mc, LkSlideBox{INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN}, true));   // (a box that holds every key)
    LKCHK(compact_count(h, &mc));
    unsigned int bad = 0, behind_roots = mc.all_nodes;   // new id of the first private CHILD record (none: the end)
    HIPCHK(h, hipMemcpyAsync(&bad, mc.cnt + 2, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    if (pn > ov.hash_cap) HIPCHK(h, hipMemcpyAsync(&behind_roots, xn_node + ov.hash_cap, sizeof(behind_roots), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const unsigned int x_roots = behind_roots - mc.live_nodes, n_roots = mc.kept_roots + x_roots;
    if (bad || x_roots != octr[LK_CTR_ROOTS]) return fail(h, LK_ERR_STATE, "the slot's overlay is not a whole map (an id outside its pools, or a root that was claimed and never made)");
    if (mc.all_nodes > h->map.max_nodes || mc.all_blocks > h->map.max_blocks || 2 * (size_t)n_roots > h->hash_cap) {
        char buf[320];
        snprintf(buf, sizeof(buf), "the committed map needs %u nodes (%u of the map's stay, %u private), %u point blocks (%u + %u) and %u root voxels (%u + %u): the handle has max_nodes %u, max_point_blocks %u and room for %u roots",
                 mc.all_nodes, mc.live_nodes, mc.all_nodes - mc.live_nodes, mc.all_blocks, mc.live_blocks, mc.all_blocks - mc.live_blocks, n_roots, mc.kept_roots, x_roots,
                 h->map.max_nodes, h->map.max_blocks, h->hash_cap / 2);
        return fail(h, LK_ERR_CAPACITY, buf);
    }
    LKCHK(compact_move(h, &mc));   // from here on the map changes: the grid is invalid, the replay's overlays are stale (ov_readable)
    // the private records behind the survivors, ids renumbered by the ranks, a private root's overlay-only words cleared; a wave per block
    LAUNCH(h, "ov_commit_nodes", hipLaunchKernelGGL(lk_slide_move_nodes_kernel, dim3((pn + 255) / 256), dim3(256), 0, h->stream, pm, pn, xa_node, xn_node, xn_block,
                                                    h->map.nodes, h->map.planes, h->map.match, 1));
    if (pb) LAUNCH(h, "ov_commit_blocks", hipLaunchKernelGGL(lk_slide_move_blocks_kernel, dim3(pb), dim3(64), 0, h->stream, pm, xa_block, xn_block, h->map.blocks));
    LAUNCH(h, "ov_commit_roots", hipLaunchKernelGGL(lk_ov_commit_roots_kernel, dim3(root_grid), dim3(256), 0, h->stream, ov, slot, xa_node, xn_node, mc.live_nodes, mc.kept + mc.kept_roots));
    if (mc.all_nodes > mc.live_nodes) {   // a lazily copied voxel's match record never was private: all appended ones are derived, as an import does
        LkMap app = h->map;
        app.planes += mc.live_nodes, app.match += mc.live_nodes;
        LAUNCH(h, "derive_match", hipLaunchKernelGGL(lk_derive_match_kernel, dim3((mc.all_nodes - mc.live_nodes + 255) / 256), dim3(256), 0, h->stream, app, (int)(mc.all_nodes - mc.live_nodes)));
    }
    LKCHK(compact_finish(h, &mc, mc.all_nodes, mc.all_blocks, n_roots, true));
    if ((flags & LK_COMMIT_ADOPT_FILTER) && slot != 0) {
        HIPCHK(h, hipMemcpyAsync(h->d_filters, h->d_filters + slot, sizeof(LkFilter), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return LK_OK;
}

// ------------------------------------------------------------------ batch replay with a per-scan insert overlay
// (lk_overlay_kernels.h) KILO::process for every scan of the batch - predict, residual, update AND map insert per bucket (KILO.cc:108-233,
// :375-395) - each scan on its own copy-on-write overlay of the handle's map, which itself stays untouched.

// The overlay arrays, one entry per pointer of LkOverlay in the order they are allocated: where the pointer lives, whether every slot owns a range of the
// array or all slots share it, and the BYTES a slot owns (shared: the bytes of the whole array) under the handle's capacities.  The one
// host-side description of the pools: ov_reserve allocates from it, ov_free releases, ov_at offsets.  The kernels' description of the same layout is ov_slot_map.
struct OvPool { size_t at; bool shared; size_t (*bytes)(const lk_handle* h); };   // at: offsetof(LkOverlay, the pointer)
#define OV_POOL(field, shared, ...) {offsetof(LkOverlay, field), shared, [](const lk_handle* h) -> size_t { const LkOverlay& c = h->ov; (void)c; return __VA_ARGS__; }}
constexpr bool kPerSlot = false, kShared = true;
static const OvPool kOvPools[] = {
    OV_POOL(keys, kPerSlot, sizeof(unsigned long long) * c.hash_cap),
    OV_POOL(planes, kPerSlot, sizeof(lk_plane_rec) * c.nodes_cap), OV_POOL(match, kPerSlot, sizeof(lk_match_rec) * c.nodes_cap), OV_POOL(nodes, kPerSlot, sizeof(lk_node_rec) * c.nodes_cap),
    OV_POOL(blocks, kPerSlot, sizeof(lk_block_rec) * c.blocks_cap),
    OV_POOL(counters, kPerSlot, sizeof(unsigned int) * LK_CTR_COUNT),
    OV_POOL(touched, kPerSlot, sizeof(int) * c.scan_cap), OV_POOL(next, kPerSlot, sizeof(int) * c.scan_cap), OV_POOL(scratch, kPerSlot, sizeof(int) * c.scan_cap), OV_POOL(gidx, kPerSlot, sizeof(int) * c.scan_cap),
    OV_POOL(groups, kPerSlot, sizeof(LkGroup) * 2 * c.scan_cap),
    OV_POOL(slots, kPerSlot, sizeof(float4) * LK_SLOTS * c.hash_cap),
    OV_POOL(free_list, kPerSlot, sizeof(int) * c.blocks_cap), OV_POOL(freed_next, kPerSlot, sizeof(int) * c.blocks_cap),
    OV_POOL(dirty, kPerSlot, sizeof(unsigned int) * c.hash_cap),
    OV_POOL(newroot, kShared, sizeof(unsigned int) * (LK_NEWROOT_MASK + 1)), OV_POOL(spec, kShared, sizeof(unsigned int) * LK_SPEC_WORDS),
    OV_POOL(bits, kPerSlot, sizeof(unsigned int) * c.bit_words),
    OV_POOL(frozen, kShared, sizeof(unsigned int) * 2 * c.bit_words),
    OV_POOL(jobs, kPerSlot, sizeof(LkFitJob) * LK_INLINE_GROUPS * c.hash_cap), OV_POOL(jobhdr, kPerSlot, sizeof(int4) * LK_INLINE_GROUPS * c.hash_cap),
    OV_POOL(sums, kPerSlot, sizeof(LkLeafSum) * c.hash_cap),
    OV_POOL(base_sums, kShared, sizeof(LkLeafSum) * h->map.max_nodes),
    OV_POOL(cplx, kPerSlot, sizeof(int) * 2 * c.scan_cap), OV_POOL(ptroot, kPerSlot, sizeof(int) * c.scan_cap),
};
#undef OV_POOL
static_assert(std::is_standard_layout<LkOverlay>::value && sizeof(LkOverlay) == (sizeof(kOvPools) / sizeof(kOvPools[0]) + 3) * sizeof(void*),
              "25 pointers and five capacities (24 B with the padding): an array added to LkOverlay needs its row in kOvPools");
// (the pointers are of 25 types: read and written as bytes)
static char* ov_pool_ptr(const LkOverlay& o, const OvPool& p) { char* q; memcpy(&q, reinterpret_cast<const char*>(&o) + p.at, sizeof(q)); return q; }
static void ov_pool_set(LkOverlay& o, const OvPool& p, void* q) { memcpy(reinterpret_cast<char*>(&o) + p.at, &q, sizeof(q)); }

void ov_free(lk_handle* h) {
    for (const OvPool& p : kOvPools)
        if (char* q = ov_pool_ptr(h->ov, p)) hipFree(q);
    memset(&h->ov, 0, sizeof(h->ov));
    h->ov_slots = 0;
    h->ov_pool_bytes = 0;
    h->ov_last_slots = 0;   // nothing of the last replay is left to export / count (lk_overlay_export, lk_overlay_stats)
}
// the overlay pools as a group of slots starting at slot s0 sees them: every per-slot array advanced by s0 slots (the kernels index by blockIdx.y)
static LkOverlay ov_at(const lk_handle* h, size_t s0) {
    LkOverlay r = h->ov;
    for (const OvPool& p : kOvPools)
        if (!p.shared) ov_pool_set(r, p, ov_pool_ptr(r, p) + s0 * p.bytes(h));
    return r;
}
// The table against the kernels' view (ov_slot_map), for fresh pools of S slots: slot b of the group that starts at slot a is slot a + b of the pools, in
// every array ov_slot_map addresses.  (keys, bits, jobs, jobhdr, sums, ptroot: the kernels index them by hand; the table and LkOverlay's comments are the record.)
static int ov_check_layout(lk_handle* h, uint32_t S) {
    const char* bad = nullptr;
    for (const uint32_t a : {S / 2, S - 1}) {
        const LkMap x = ov_slot_map(ov_at(h, a), S - 1 - a), y = ov_slot_map(h->ov, S - 1);
#define OV_SAME(f) if (x.f != y.f) bad = #f;
        OV_SAME(planes) OV_SAME(match) OV_SAME(nodes) OV_SAME(blocks) OV_SAME(counters) OV_SAME(touched) OV_SAME(heavy) OV_SAME(next) OV_SAME(slots)
        OV_SAME(scratch) OV_SAME(groups) OV_SAME(gidx) OV_SAME(free_list) OV_SAME(freed_next) OV_SAME(dirty) OV_SAME(newroot) OV_SAME(spec)
#undef OV_SAME
    }
    return bad ? fail(h, LK_ERR_STATE, std::string("overlay pools: the host's table (ov_at) and ov_slot_map disagree on LkMap::") + bad) : LK_OK;
}
// LEGKILO_POISON_POOLS (test aid): node records that look plausible - a few points, no children - and point at a block far outside any pool
__global__ void __launch_bounds__(256) lk_ov_poison_nodes_kernel(lk_node_rec* nodes, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    nodes[i].npts = 3, nodes[i].new_points = 1, nodes[i].block = 0x3fffff00, nodes[i].layer = 0, nodes[i].state = LK_NODE_UPDATE_ENABLE | LK_NODE_INIT_OCTO;
    for (int c = 0; c < 8; ++c) nodes[i].child[c] = -1;
}
// Per-scan capacities.  lk_overlay_reserve's numbers if given; else, when an earlier replay of scans of this size has left its
// high-water marks, those + 25 % (pools more than twice that are released and re-made: round 4 reserved n_pts / 6 roots = 110 MB per scan,
// 113 GB for 1 024 scans, where the bench's scans use 4 700 roots); else a first guess of n_pts / 18 roots.  `grow` (bits of the slots' error
// word: 1 private root table, 2 nodes, 4 point blocks) doubles what overflowed - the replay is then run again (ov_replay).
static int ov_reserve(lk_handle* h, uint32_t S, size_t n_pts_scan, size_t biggest_bucket, const LkMap& fmap, unsigned int grow = 0) {
    // (a run and a single scan of equal point count are not the same shape: a run's overlay keeps growing over its scans)
    const bool hist = h->ov_hw_roots > 0 && h->ov_hw_npts == n_pts_scan && h->ov_hw_runs == h->ov_runs;
    uint32_t roots, nodes_extra, blocks;
    if (h->ov_want_roots) {
        roots = h->ov_want_roots;
        nodes_extra = h->ov_want_nodes ? std::max(h->ov_want_nodes, roots + 64u) - roots : roots / 2;
        blocks = h->ov_want_blocks ? h->ov_want_blocks : roots;
    } else if (hist) {
        roots = h->ov_hw_roots + h->ov_hw_roots / 4 + 64;
        const uint32_t child = h->ov_hw_nodes > h->ov_hw_roots ? h->ov_hw_nodes - h->ov_hw_roots : 0u;
        nodes_extra = child + child / 4 + 256;
        blocks = h->ov_hw_blocks + h->ov_hw_blocks / 4 + 64;
    } else {
        roots = (uint32_t)std::min<size_t>(std::max<size_t>(2048, n_pts_scan / 18), std::max<size_t>(1024, n_pts_scan));
        nodes_extra = roots / 2;
        blocks = roots;
    }
    uint32_t hash_cap = next_pow2(roots + roots / 4);       // the roots' records ARE the table entries: node ids [0, hash_cap); load <= 0.8 (0.57 for the bench's scans)
    LkOverlay& o = h->ov;
    if (grow) {   // never below what is there; what overflowed is doubled
        hash_cap = std::max(hash_cap, o.hash_cap), nodes_extra = std::max(nodes_extra, o.nodes_cap - o.hash_cap), blocks = std::max(blocks, o.blocks_cap);
        if (grow & LK_E_HASH_FULL) {
            // A scan that cannot claim its roots stops there: the blocks and child nodes of the roots it did not get are never asked for, so an
            // attempt whose table overflows reports the table alone.  Doubling one pool per attempt spent the four attempts on the table and left
            // none for the point blocks (history-sized pools of a 10-voxel scan, then a 600-voxel scan: LK_ERR_CAPACITY at 1024 entries / 152 blocks).
            // The first guess's proportions go with the table instead: roots = 4/5 of its entries, a block per root, a child node per two.
            hash_cap *= 2;
            const uint32_t r = hash_cap / 5 * 4;
            blocks = std::max(blocks, r), nodes_extra = std::max(nodes_extra, r / 2);
        }
        if (grow & LK_E_NODES_FULL) nodes_extra = nodes_extra * 2 + 256;
        if (grow & LK_E_BLOCKS_FULL) blocks *= 2;
    }
    const uint32_t nodes_cap = hash_cap + nodes_extra;        // children from hash_cap upwards
    const uint32_t scan_cap = (uint32_t)((biggest_bucket + 63) & ~(size_t)63);
    const size_t cells = (size_t)fmap.gdim[0] * (size_t)fmap.gdim[1] * (size_t)fmap.gdim[2];
    const uint32_t bit_words = (uint32_t)((cells + 31) / 32);
    const bool fits = S <= h->ov_slots && hash_cap <= o.hash_cap && nodes_cap - hash_cap <= o.nodes_cap - o.hash_cap && blocks <= o.blocks_cap &&
                      scan_cap <= o.scan_cap && bit_words <= o.bit_words;
    // far too large for what the scans use (measured by an earlier replay, or asked for explicitly): released and re-made
    const bool oversized = (hist || h->ov_want_roots) && !grow && (o.hash_cap > 2 * hash_cap || (size_t)o.blocks_cap > 2 * (size_t)blocks + 1024);
    if (fits && !oversized) return LK_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint32_t S2 = oversized ? S : std::max(S, h->ov_slots);
    LkOverlay n = {};
    if (oversized) {
        n.hash_cap = hash_cap, n.nodes_cap = nodes_cap, n.blocks_cap = blocks, n.scan_cap = scan_cap, n.bit_words = bit_words;
    } else {
        n.hash_cap = std::max(hash_cap, o.hash_cap);
        n.nodes_cap = n.hash_cap + std::max(nodes_extra, o.nodes_cap > o.hash_cap ? o.nodes_cap - o.hash_cap : 0u);
        n.blocks_cap = std::max(blocks, o.blocks_cap), n.scan_cap = std::max(scan_cap, o.scan_cap), n.bit_words = std::max(bit_words, o.bit_words);
    }
    ov_free(h);
    h->ov = n;
    const size_t s = S2;
    size_t total = 0;
    hipError_t e = hipSuccess;
    for (const OvPool& p : kOvPools) {
        const size_t bytes = (p.shared ? 1 : s) * p.bytes(h);
        void* q = nullptr;
        total += bytes;
        if ((e = hipMalloc(&q, bytes)) != hipSuccess) break;
        ov_pool_set(o, p, q);
    }
    if (e == hipSuccess && !h->d_ov_status) e = pool_alloc(h, &h->d_ov_status, 8 * sizeof(unsigned int));
    if (e == hipSuccess && lk_poison_pools()) {
        // test aid: fresh pools hold 0x5a bytes instead of whatever the allocator hands out (usually zeros) - a kernel that trusts a record
        // nobody has written then faults HERE AND NOW, not in the one process whose allocation history leaves garbage there
        hipLaunchKernelGGL(lk_ov_poison_nodes_kernel, dim3((unsigned int)((s * n.nodes_cap + 255) / 256)), dim3(256), 0, h->stream, o.nodes, s * n.nodes_cap);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ov_free(h);
        char buf[256];
        snprintf(buf, sizeof(buf), "overlay pools for %u scans (%u root entries / %u child nodes / %u point blocks each) do not fit: %s (lk_overlay_reserve sets smaller per-scan capacities)",
                 S2, n.hash_cap, n.nodes_cap - n.hash_cap, n.blocks_cap, hipGetErrorString(e));
        return fail(h, LK_ERR_CAPACITY, buf);
    }
    if (const int rc = ov_check_layout(h, S2)) {   // pools that the kernels would address differently are not kept: the next call fails here again
        ov_free(h);
        return rc;
    }
    h->ov_slots = S2;
    h->ov_pool_bytes = total;
    hipLaunchKernelGGL(lk_ov_init_kernel, dim3((n.hash_cap + 255) / 256, S2), dim3(256), 0, h->stream, h->ov);
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}

int lk_overlay_reserve(lk_handle* h, uint32_t roots_per_scan, uint32_t nodes_per_scan, uint32_t blocks_per_scan) {
    CHECK_H(h);
    if ((roots_per_scan && roots_per_scan < 16) || (nodes_per_scan && nodes_per_scan < roots_per_scan) || (blocks_per_scan && blocks_per_scan < 16))
        return fail(h, LK_ERR_INVALID, "overlay capacities too small (0 = derive from the scan size)");
    h->ov_want_roots = roots_per_scan, h->ov_want_nodes = nodes_per_scan, h->ov_want_blocks = blocks_per_scan;
    if (h->ov_slots) {   // pools of another shape are released; the next replay allocates what it needs
        HIPCHK(h, hipStreamSynchronize(h->stream));
        ov_free(h);
    }
    return LK_OK;
}

}  // extern "C"
// ---- what the replays with insert share (lk_batch_replay_overlay_dev, overlay_ragged_launch): ov_replay, the scaffold around an attempt's launches.
// A scan whose overlay outgrows pools that were sized by this library (first guess, or the previous replay's high-water marks) makes the
// pools grow and the whole batch run again from its priors - only capacities the caller has set explicitly (lk_overlay_reserve) fail with
// LK_ERR_CAPACITY.

// The residual pass with the overlay lookup, specialised for ext_R == I where it holds (LEGKILO_XID=0: the generic one).
static auto ov_residual_kernel(const lk_handle* h) {
    return (h->pr.ext_identity && lk_xid_enabled()) ? lk_ov_residual_kernel<true> : lk_ov_residual_kernel<false>;
}
// Before the first attempt: the frozen map with its grid, pools for S scans of n_pts_scan points, the batch's priors put aside.
static int ov_replay_begin(lk_handle* h, int S, size_t n_pts_scan, size_t biggest, LkMap* fmap) {
    LKCHK(join_side_streams(h));   // an asynchronous frozen-map batch may still be using the filter slots
    LKCHK(frozen_map(h, fmap));
    if (!fmap->grid_on) return fail(h, LK_ERR_STATE, "overlay replay needs the frozen-map grid (root keys' bounding box too large, LEGKILO_GRID=0, or out of device memory)");
    LKCHK(ov_reserve(h, (uint32_t)S, n_pts_scan, biggest, *fmap));
    LKCHK(reserve(h, h->ov_priors, sizeof(LkFilter) * (size_t)S));
    HIPCHK(h, hipMemcpyAsync(h->ov_priors.p, h->d_filters, sizeof(LkFilter) * (size_t)S, hipMemcpyDeviceToDevice, h->stream));
    return LK_OK;
}
// Head of an attempt: scan counters, start times (d_tbegin: one per scan; null: t_begin for all), the frozen bits and the base map's leaf sums.
static int ov_attempt_begin(lk_handle* h, int S, const LkMap& fmap, const double* d_tbegin, double t_begin) {
    const LkOverlay& ov = h->ov;
    hipStream_t st = h->stream;
    LKCHK(zero_scan_counters(h, 0, (uint32_t)S));
    if (d_tbegin) hipLaunchKernelGGL(lk_set_times_ragged_kernel, dim3((S + 63) / 64), dim3(64), 0, st, h->d_filters, S, d_tbegin);
    else hipLaunchKernelGGL(lk_set_times_kernel, dim3((S + 63) / 64), dim3(64), 0, st, h->d_filters, S, t_begin);
    HIPCHK(h, hipMemsetAsync(ov.frozen, 0, (size_t)2 * ov.bit_words * sizeof(unsigned int), st));
    // both bits of every cell (LkOverlay::frozen): frozen leaf, and takes the point at the root
    LAUNCH(h, "ov_frozen_bits", hipLaunchKernelGGL(lk_ov_frozen_bits_kernel, dim3((h->hash_cap + 255) / 256), dim3(256), 0, st, fmap, h->hash_cap, h->pr.max_layer, ov.frozen, 1));
    LAUNCH(h, "ov_base_sums", hipLaunchKernelGGL(lk_ov_base_sums_kernel, dim3((h->hash_cap + 255) / 256), dim3(256), 0, st, fmap, h->hash_cap, ov.base_sums));
    return LK_OK;
}
// The status words of the first S slots' overlays: [0] error bits of any slot, [1..3] largest use of nodes / blocks / roots, [4] first slot with an error.  Synchronises.
static int ov_read_status(lk_handle* h, unsigned int S, unsigned int* stt) {
    const unsigned int init[8] = {0u, 0u, 0u, 0u, 0xffffffffu, 0u, 0u, 0u};
    HIPCHK(h, hipMemcpyAsync(h->d_ov_status, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(lk_ov_status_kernel, dim3(std::min((S + 255u) / 256u, 64u)), dim3(256), 0, h->stream, h->ov, S, h->d_ov_status);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(stt, h->d_ov_status, 8 * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}
// Tail of an attempt, from its status.  *again: pools the library sized have overflowed - they have grown, the priors are back, run the
// attempt once more.  Otherwise the replay is over: high-water marks for the next one's pools, the poses, and the slots' errors if any.
static int ov_attempt_end(lk_handle* h, int S, int attempt, const unsigned int* stt, size_t n_pts_scan, size_t biggest, const LkMap& fmap, lk_pose* out, bool* again) {
    const bool growable = !h->ov_want_roots && !(stt[0] & ~(LK_E_HASH_FULL | LK_E_NODES_FULL | LK_E_BLOCKS_FULL)) && attempt < 4;
    *again = stt[0] && growable;
    if (!stt[0]) h->ov_hw_roots = stt[3], h->ov_hw_nodes = stt[1], h->ov_hw_blocks = stt[2], h->ov_hw_npts = n_pts_scan, h->ov_hw_runs = h->ov_runs;
    if (out && !*again) LKCHK(fetch_poses(h, out, S));   // no wait without `out`: ov_read_status has synchronised
    // the priors are back whenever a slot has reported an error: the next attempt starts from them, and a refused replay leaves the slots as the
    // caller armed them, not at whatever the buckets before the error made of them
    if (stt[0]) HIPCHK(h, hipMemcpyAsync(h->d_filters, h->ov_priors.p, sizeof(LkFilter) * (size_t)S, hipMemcpyDeviceToDevice, h->stream));
    if (*again) return ov_reserve(h, (uint32_t)S, n_pts_scan, biggest, fmap, stt[0]);
    if (stt[0] & LK_E_KEY_RANGE) {
        char buf[200];
        snprintf(buf, sizeof(buf), "overlay replay: a point of slot %u lies in a voxel whose key is outside the +-2^20 range of the private root tables' packed keys (%.0f km from the origin at this voxel size)",
                 stt[4], 1048576.0 * h->cfg.max_voxel_size / 1000.0);
        return fail(h, LK_ERR_INVALID, buf);
    }
    if (stt[0]) {
        const LkOverlay& ov = h->ov;
        char buf[256];
        snprintf(buf, sizeof(buf), "overlay pool overflow in slot %u (bits 0x%x: 1 private root table, 2 nodes, 4 point blocks, 8 work lists); largest use over the slots: %u nodes, %u blocks, %u roots; per-scan pools: %u root entries, %u child nodes, %u blocks (lk_overlay_reserve)",
                 stt[4], stt[0], stt[1], stt[2], stt[3], ov.hash_cap, ov.nodes_cap - ov.hash_cap, ov.blocks_cap);
        return fail(h, LK_ERR_CAPACITY, buf);
    }
    return LK_OK;
}

// A whole replay with insert: the attempt loop around `enqueue(fmap)`, which puts ONE attempt's launches behind ov_attempt_begin's - reset of the
// overlays included - and returns once they are enqueued (an error: the replay returns it, no status is read).  The entries differ in nothing else.
template <class Enqueue>
static int ov_replay(lk_handle* h, int S, size_t n_pts_scan, size_t biggest, const double* d_tbegin, double t_begin, lk_pose* out, Enqueue&& enqueue) {
    LkMap fmap;
    LKCHK(ov_replay_begin(h, S, n_pts_scan, biggest, &fmap));
    h->bucket_n = 0;   // (the _cloud entry sets it behind its replay)
    for (int attempt = 0;; ++attempt) {
        LKCHK(ov_attempt_begin(h, S, fmap, d_tbegin, t_begin));
        LKCHK(enqueue(fmap));
        h->ov_last_slots = (uint32_t)S, h->ov_gen = h->map_gen;
        unsigned int stt[8];
        LKCHK(ov_read_status(h, (unsigned int)S, stt));
        bool again = false;
        const int rc = ov_attempt_end(h, S, attempt, stt, n_pts_scan, biggest, fmap, out, &again);
        if (!again) return rc;
        LKCHK(rc);
    }
}
static int ov_reset(lk_handle* h, hipStream_t st, const LkOverlay& ov, int Sg) {
    const unsigned int per = std::max(std::max(ov.hash_cap, ov.bit_words), (unsigned int)LK_CTR_COUNT);   // root records, bitmap words, counters
    LAUNCH(h, "ov_reset", hipLaunchKernelGGL(lk_ov_reset_kernel, dim3((per + 255) / 256, Sg), dim3(256), 0, st, ov));
    return LK_OK;
}

// The insert of one bucket into the overlays of Sg slots from its posterior (KILO.cc:216-233), on stream st: ov_begin ... ov_insert_apply; the
// fallback launch behind them is the caller's.  nb: the (longest) bucket's points; S: the slots of the whole batch, which size the per-root passes.
// Two launch shapes differ between the callers, each as measured for its entry:
//   min_root_lane: workgroups per slot of lk_ov_root_lane_kernel at least - 4 in the uniform batch, 1 in the ragged one (as measured for this entry; not re-swept);
//   fit_blocks:    waves per scan of the two fit passes - 12 in the uniform batch (round 6, job headers in a dense array: 6 / 8 / 12 / 16 / 24 waves
//                  -> fit pass 1.75 / 1.92 / 1.61 / 2.12 / 1.71 ms; before: best at 6, 1.89), min(8, (nb + 63) / 64) in the ragged one (as measured
//                  for this entry; not re-swept).
static int ov_insert_passes(lk_handle* h, hipStream_t st, const LkMap& fmap, const LkOverlay& ov, LkFilter* fl, const LkPtSrc& src, int nb, int S, int Sg,
                            int min_root_lane, int fit_blocks) {
    LAUNCH(h, "ov_begin", hipLaunchKernelGGL(lk_ov_begin_kernel, dim3(Sg), dim3(LK_WAVE), 0, st, ov));
    LAUNCH(h, "ov_reproject", hipLaunchKernelGGL(lk_ov_reproject_kernel, dim3((nb + LK_WAVE - 1) / LK_WAVE, Sg), dim3(LK_WAVE), 0, st, fmap, ov, h->pr, fl, src));
    // per-root passes: enough waves per slot to cover its touched roots a few at a time, ~4096 workgroups per launch at least
    const int per_slot = std::max(1, std::min((nb + 255) / 256, std::max(2, (4096 + S - 1) / S)));
    // (measured at 1024 slots x 20 000-point buckets, workgroups per slot: copy-on-write 2.8 / 6.6 / 12.2 ms per batch at 4 / 16 / 32 - a wave takes 64
    // roots, more waves only find nothing to do; root pass 12.8 / 11.0 / 11.7 - a wave works through its roots one after the other)
    LAUNCH(h, "ov_materialise", hipLaunchKernelGGL(lk_ov_materialise_kernel<true>, dim3(std::max(1, per_slot / 2), Sg), dim3(LK_MB), 0, st, fmap, ov, h->pr));
    // root pass: one thread per point (geometry) + one lane per root (lk_ov_point_geom_kernel, lk_ov_root_lane_kernel: root leaves that append / refit /
    // freeze), then the generic pass over what they leave - three waves per SIMD (without the fit: 184 VGPRs at 2 waves, 168 at 3) - with the
    // leaf's plane fit only decided; then the fits, a group of lanes each
    LAUNCH(h, "ov_point_geom", hipLaunchKernelGGL(lk_ov_point_geom_kernel, dim3((nb + 255) / 256, Sg), dim3(256), 0, st, ov, h->pr, fl, src));
    LAUNCH(h, "ov_root_lane", hipLaunchKernelGGL(lk_ov_root_lane_kernel, dim3(std::max(min_root_lane, (nb + 16 * LK_WAVE - 1) / (16 * LK_WAVE)), Sg), dim3(LK_WAVE), 0, st, fmap, ov, h->pr));
    LAUNCH(h, "ov_insert_root", hipLaunchKernelGGL((lk_ov_insert_root_kernel<3, true>), dim3(std::max(1, per_slot / 2), Sg), dim3(LK_MB), 0, st, fmap, ov, h->pr, fl, src));
    LAUNCH(h, "ov_fit_eig", hipLaunchKernelGGL(lk_ov_fit_eig_kernel, dim3(fit_blocks, Sg), dim3(LK_WAVE), 0, st, fmap, ov, h->pr));
    LAUNCH(h, "ov_fit_lane", hipLaunchKernelGGL(lk_ov_fit_group_kernel, dim3(fit_blocks, Sg), dim3(LK_WAVE), 0, st, fmap, ov, h->pr));
    LAUNCH(h, "ov_insert_apply", hipLaunchKernelGGL(lk_ov_insert_apply_kernel, dim3(per_slot, Sg), dim3(LK_MB), 0, st, ov, h->pr, fl, src));
    return LK_OK;
}

// An attempt's launches of the uniform batch: bucket after bucket, every slot group's launches of it on the group's stream.
// Four slot groups on separate HIP streams (round 6, same box: 15.14 / 13.48 / 13.02 / 12.74 ms with 1 / 2 / 3 / 4 groups, 14.8 / 14.2 with
// 6 / 8: beyond four streams the queues share hardware): the passes of a bucket are of two kinds - the root pass issues VALU work at
// 2.8 TB/s of HBM traffic, the others (re-projection, copy-on-write, plane fits) only move bytes - so one group's root pass runs beside
// the other group's memory passes.  A group is the same launches with every per-slot array offset to its first slot (ov_at).
static int ov_uniform_launches(lk_handle* h, const SlotGroups& grp, const LkMap& fmap, const lk_point* d_pts, size_t n_pts, double t_begin, const uint32_t* bucket_off,
                               const double* bucket_dt, const std::vector<size_t>& live) {
    const auto res_kernel = ov_residual_kernel(h);
    for (int g = 0; g < grp.n; ++g) LKCHK(ov_reset(h, grp.stream[g], ov_at(h, (size_t)grp.first(g)), grp.count(g)));
    for (size_t k = 0; k < live.size(); ++k)
        for (int g = 0; g < grp.n; ++g) {
            const int s0 = grp.first(g), Sg = grp.count(g);   // this group's slots
            const LkOverlay ov = ov_at(h, (size_t)s0);
            hipStream_t st = grp.stream[g];
            LkFilter* fl = h->d_filters + s0;
            double* parts = h->d_partials + (size_t)s0 * h->part_stride;
            const size_t b = live[k];
            const int nb = (int)(bucket_off[b + 1] - bucket_off[b]);
            const double t = t_begin + bucket_dt[b];
            const int nblk = (nb + LK_RB - 1) / LK_RB;
            const LkPtSrc src = {d_pts + (size_t)s0 * n_pts + bucket_off[b], n_pts, nb, nullptr, nullptr, 0, 0, nullptr};
            if (k == 0) LAUNCH(h, "predict", hipLaunchKernelGGL(lk_update_wave_kernel, dim3(Sg), dim3(LK_WAVE), 0, st, fl, parts, 0, h->part_stride, 0.0, h->d_Q, t, 2));
            LAUNCH(h, "ov_residual", hipLaunchKernelGGL(res_kernel, dim3(nblk, Sg), dim3(LK_RB), 0, st, fmap, ov, h->pr, fl, src, parts, h->part_stride));
            LAUNCH(h, "update", hipLaunchKernelGGL(lk_update_wave_kernel, dim3(Sg), dim3(LK_WAVE), 0, st, fl, parts, nblk * (LK_RB / LK_WAVE), h->part_stride, t, h->d_Q, 0.0, 1));
            LKCHK(ov_insert_passes(h, st, fmap, ov, fl, src, nb, grp.S, Sg, 4, 12));
            LAUNCH(h, "ov_insert_fallback", hipLaunchKernelGGL(lk_ov_insert_fallback_kernel, dim3(std::min(Sg, 128)), dim3(LK_MB), 0, st, ov, h->pr, fl, src, Sg));   // (1 024 slots, workgroups 8 / 32 / 128 / 256 / 512: 0.54 / 0.26 / 0.15 / 0.17 / 0.16 ms per batch; a workgroup or more per slot: 0.34)
            if (k + 1 < live.size())
                LAUNCH(h, "predict", hipLaunchKernelGGL(lk_update_wave_kernel, dim3(Sg), dim3(LK_WAVE), 0, st, fl, parts, 0, h->part_stride, 0.0, h->d_Q,
                                                        t_begin + bucket_dt[live[k + 1]], 2));
        }
    HIPCHK(h, hipGetLastError());
    return LK_OK;
}

extern "C" {
int lk_batch_replay_overlay_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, size_t n_pts, double t_begin, const uint32_t* bucket_off,
                                const double* bucket_dt, size_t n_buckets, lk_pose* out) {
    CHECK_H(h);
    if (n_scans == 0 || n_scans > h->cfg.n_slots) return fail(h, LK_ERR_INVALID, "n_scans must be in [1, n_slots]");
    if (n_pts == 0 || n_buckets == 0) return fail(h, LK_ERR_INVALID, "empty scans");
    if (!d_pts || !bucket_off || !bucket_dt) return fail(h, LK_ERR_INVALID, "null argument");
    const int S = (int)n_scans;
    h->ov_runs = false;
    std::vector<size_t> live;
    size_t biggest = 0;
    // this entry's own checks, bucket by bucket ahead of the shared one: the first bad bucket decides which error the caller sees
    LKCHK(live_buckets(h, bucket_off, n_buckets, live, &biggest, [&](size_t b) -> int {
        if (bucket_off[b + 1] < bucket_off[b] || bucket_off[b + 1] > n_pts) return fail(h, LK_ERR_INVALID, "bucket offsets must be non-decreasing and end inside the scan");
        if (!std::isfinite(bucket_dt[b]) || (b > 0 && bucket_dt[b] < bucket_dt[b - 1])) return fail(h, LK_ERR_INVALID, "bucket times must be finite and non-decreasing");
        return LK_OK;
    }));
    if (live.empty()) return fail(h, LK_ERR_INVALID, "empty scans");
    const SlotGroups grp(h, S, kOverlayGroups, kOverlayGroupSlots);
    return ov_replay(h, S, n_pts, biggest, nullptr, t_begin, out, [&](const LkMap& fmap) -> int {
        LKCHK(grp.fork());
        return grp.join(ov_uniform_launches(h, grp, fmap, d_pts, n_pts, t_begin, bucket_off, bucket_dt, live));
    });
}

int lk_batch_replay_overlay_ragged_dev(lk_handle* h, const lk_point* d_pts, size_t n_scans, const uint64_t* scan_off, const uint32_t* n_buckets,
                                       const uint32_t* bucket_off, const double* bucket_dt, const double* t_begin, const uint32_t* n_msg, const void* msgs,
                                       int msg_kind, lk_pose* out) {
    CHECK_H(h);
    if (msg_kind < 0 || msg_kind > 2) return fail(h, LK_ERR_INVALID, "msg_kind must be 0 (no messages), 1 (lk_imu) or 2 (lk_kin_imu)");
    if (msg_kind && !n_msg) return fail(h, LK_ERR_INVALID, "null argument");
    return ragged_replay(h, d_pts, n_scans, scan_off, n_buckets, bucket_off, bucket_dt, t_begin, msg_kind ? n_msg : nullptr, msgs, msg_kind, out, true);
}
}  // extern "C"
// The ragged batch WITH insert on one stream (a recorded run's buckets are small, the launches are what it costs): behind the reset of the overlays an
// attempt's launches go one of three ways.  Runs (rg.run_scan, CSR tables: lk_batch_replay_overlay_runs_dev): a slot is a run of scans - for addressing and
// time one long scan of ldb buckets at most, max_scan_pts its points; the kernels know where its scans end (rag_bucket), and `out` takes the n_poses
// records of rg.scan_pose instead of the slots' poses.
// 1. Buckets of <= LK_SCAN_WAVE_MAX points, scan-resident: one wave per scan (run) works through its buckets in ONE launch (lk_ovscan.hip, lk_ovrun.hip) and
// stops where a bucket leaves fallback items; those run as a launch of their own, then the resident kernel picks every stopped scan up again.
static int ov_rag_resident_rounds(lk_handle* h, int S, const LkMap& fmap, const LkRagged& rg, const lk_point* d_pts, int msg_kind, size_t ldb) {
    hipStream_t st = h->stream;
    const bool xid = h->pr.ext_identity && lk_xid_enabled(), runs = rg.run_scan != nullptr;
    // [S] next bucket of every scan, [S] the bucket whose fallback items wait, one counter: scans stopped by fallback items in the last launch
    LKCHK(reserve(h, h->ov_res, sizeof(int) * (2 * (size_t)S + 4)));
    int* cur = static_cast<int*>(h->ov_res.p);
    int* fb_b = cur + S;
    unsigned int* pending = reinterpret_cast<unsigned int*>(cur + 2 * (size_t)S);
    HIPCHK(h, hipMemsetAsync(cur, 0, sizeof(int) * (2 * (size_t)S + 4), st));
    const LkPtSrc fsrc = {d_pts, 0, 0, rg.pt_off, rg.nb, rg.ldb, 0, fb_b, rg.bstart};
    unsigned int rounds = 0;
    for (;; ++rounds) {
        if (runs) LKCHK(ov_run_launch(h, xid, S, st, fmap, h->ov, h->d_filters, rg, d_pts, msg_kind, cur, fb_b, pending));   // lk_ovrun.hip
        else LKCHK(ov_scan_launch(h, xid, S, st, fmap, h->ov, h->d_filters, rg, d_pts, msg_kind, cur, fb_b, pending));   // lk_ovscan.hip
        unsigned int n_pending = 0;
        HIPCHK(h, hipMemcpyAsync(&n_pending, pending, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        if (!n_pending) break;
        if (rounds > ldb + 1) return fail(h, LK_ERR_STATE, "scan-resident overlay replay: more fallback rounds than buckets");
        HIPCHK(h, hipMemsetAsync(pending, 0, sizeof(unsigned int), st));
        LAUNCH(h, "ov_insert_fallback", hipLaunchKernelGGL(lk_ov_insert_fallback_kernel, dim3(std::min(S, 128)), dim3(LK_MB), 0, st, h->ov, h->pr, h->d_filters, fsrc, S));
    }
    h->ov_res_rounds = rounds + 1;
    return LK_OK;
}
// 2. The same buckets launch by launch, bucket INDEX after bucket index over all scans (a scan that has run out of buckets leaves every launch at once): front
// (the scan's messages up to the bucket's time, predict, residual, update, re-projection), mid, tail - at one wave per slot: 29.2 -> 26.4 ms against four launches.
static int ov_rag_small_launches(lk_handle* h, int S, const LkMap& fmap, const LkRagged& rg, const lk_point* d_pts, int msg_kind, size_t ldb) {
    const LkOverlay& ov = h->ov;
    const auto front = (h->pr.ext_identity && lk_xid_enabled()) ? lk_rag_ov_front_kernel<true> : lk_rag_ov_front_kernel<false>;
    for (size_t b = 0; b < ldb; ++b) {
        const LkPtSrc src = {d_pts, 0, 0, rg.pt_off, rg.nb, rg.ldb, (int)b, nullptr, rg.bstart};
        LAUNCH(h, "rag_ov_front", hipLaunchKernelGGL(front, dim3(S), dim3(LK_WAVE), 0, h->stream, fmap, ov, h->pr, h->d_filters, h->d_Q, rg, d_pts, (int)b, msg_kind));
        if (rg.run_scan && rg.bucket_pose) LAUNCH(h, "rag_bucket_tap", hipLaunchKernelGGL(lk_rag_bucket_tap_kernel, dim3(S), dim3(LK_WAVE), 0, h->stream, h->d_filters, rg, (int)b));
        LAUNCH(h, "ov_mid", hipLaunchKernelGGL(lk_ov_mid_kernel<true>, dim3(S), dim3(LK_MB), 0, h->stream, fmap, ov, h->pr, h->d_filters, src));
        LAUNCH(h, "ov_tail", hipLaunchKernelGGL(lk_ov_tail_kernel, dim3(S), dim3(LK_WAVE), 0, h->stream, fmap, ov, h->pr, h->d_filters, src));
        LAUNCH(h, "ov_insert_fallback", hipLaunchKernelGGL(lk_ov_insert_fallback_kernel, dim3(std::min(S, 128)), dim3(LK_MB), 0, h->stream, ov, h->pr, h->d_filters, src, S));
    }
    return LK_OK;
}
// 3. Larger buckets, index after index: lk_rag_advance_kernel, then the chain of lk_batch_replay_overlay_dev on each scan's own bucket (LkPtSrc), grids sized
// by that index's longest bucket (max_n; null: `biggest` for all); runs: the pose tap behind the update.
static int ov_rag_large_launches(lk_handle* h, int S, const LkMap& fmap, const LkRagged& rg, const lk_point* d_pts, int msg_kind, size_t ldb, const int* max_n, int biggest) {
    const LkOverlay& ov = h->ov;
    const auto res_kernel = ov_residual_kernel(h);
    for (size_t b = 0; b < ldb; ++b) {
        const int nb = std::max(1, max_n ? max_n[b] : biggest);
        const LkPtSrc src = {d_pts, 0, 0, rg.pt_off, rg.nb, rg.ldb, (int)b, nullptr, rg.bstart};
        const int nblk = (nb + LK_RB - 1) / LK_RB;
        LAUNCH(h, "rag_advance", hipLaunchKernelGGL(lk_rag_advance_kernel, dim3(S), dim3(LK_WAVE), 0, h->stream, h->d_filters, h->d_Q, rg, (int)b, msg_kind));
        LAUNCH(h, "ov_residual", hipLaunchKernelGGL(res_kernel, dim3(nblk, S), dim3(LK_RB), 0, h->stream, fmap, ov, h->pr, h->d_filters, src, h->d_partials, h->part_stride));
        LAUNCH(h, "update", hipLaunchKernelGGL(lk_update_wave_ragged_kernel, dim3(S), dim3(LK_WAVE), 0, h->stream, h->d_filters, h->d_partials, h->part_stride, h->d_Q, rg, (int)b, 1));
        if (rg.run_scan) LAUNCH(h, "rag_pose_tap", hipLaunchKernelGGL(lk_rag_pose_tap_kernel, dim3(S), dim3(LK_WAVE), 0, h->stream, h->d_filters, rg, (int)b));
        if (rg.run_scan && rg.bucket_pose) LAUNCH(h, "rag_bucket_tap", hipLaunchKernelGGL(lk_rag_bucket_tap_kernel, dim3(S), dim3(LK_WAVE), 0, h->stream, h->d_filters, rg, (int)b));
        LKCHK(ov_insert_passes(h, h->stream, fmap, ov, h->d_filters, src, nb, S, S, 1, std::max(1, std::min(8, (nb + 63) / 64))));
        LAUNCH(h, "ov_insert_fallback", hipLaunchKernelGGL(lk_ov_insert_fallback_kernel, dim3(std::min(S, 128)), dim3(LK_MB), 0, h->stream, ov, h->pr, h->d_filters, src, S));
    }
    return LK_OK;
}
int overlay_ragged_launch(lk_handle* h, const lk_point* d_pts, size_t S_, const LkRagged& rg, const double* d_tbegin, int biggest, size_t ldb,
                                 const int* max_n, size_t max_scan_pts, int msg_kind, lk_pose* out, size_t n_poses) {
    const int S = (int)S_;
    const bool runs = rg.run_scan != nullptr, small = biggest <= LK_SCAN_WAVE_MAX;
    h->ov_runs = runs;
    LKCHK(ov_replay(h, S, max_scan_pts, (size_t)biggest, d_tbegin, 0.0, runs ? nullptr : out, [&](const LkMap& fmap) -> int {
        LKCHK(ov_reset(h, h->stream, h->ov, S));
        const bool rag_resident = getenv("LEGKILO_RAG_RESIDENT") == nullptr || atoi(getenv("LEGKILO_RAG_RESIDENT")) != 0;   // 0: launch by launch (the bit-identity reference of the tests: read at every call)
        h->ov_res_rounds = 0;
        if (rag_resident && small && (!rg.bstart || runs)) LKCHK(ov_rag_resident_rounds(h, S, fmap, rg, d_pts, msg_kind, ldb));
        else if (small) LKCHK(ov_rag_small_launches(h, S, fmap, rg, d_pts, msg_kind, ldb));
        else LKCHK(ov_rag_large_launches(h, S, fmap, rg, d_pts, msg_kind, ldb, max_n, biggest));
        HIPCHK(h, hipGetLastError());
        return LK_OK;
    }));
    if (runs && out) {   // the scans' poses, written where each scan ended (the replay has synchronised)
        HIPCHK(h, hipMemcpyAsync(out, rg.scan_pose, sizeof(lk_pose) * n_poses, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return LK_OK;
}
extern "C" {
int lk_overlay_stats(lk_handle* h, uint32_t* max_roots, uint32_t* max_nodes, uint32_t* max_blocks) {
    CHECK_H(h);
    if (!h->ov_last_slots || !h->ov.counters) return fail(h, LK_ERR_STATE, "no overlay replay's pools are held by this handle (none has run, or lk_overlay_reserve released them)");
    unsigned int stt[8];
    LKCHK(ov_read_status(h, h->ov_last_slots, stt));
    if (max_nodes) *max_nodes = stt[1];
    if (max_blocks) *max_blocks = stt[2];
    if (max_roots) *max_roots = stt[3];
    return LK_OK;
}

int lk_overlay_resident_rounds(lk_handle* h, uint32_t* rounds) {
    CHECK_H(h);
    if (rounds) *rounds = h->ov_res_rounds;
    return LK_OK;
}

int lk_overlay_pool_bytes(lk_handle* h, uint64_t* bytes, uint32_t* root_entries, uint32_t* child_nodes, uint32_t* blocks) {
    CHECK_H(h);
    if (bytes) *bytes = (uint64_t)h->ov_pool_bytes;
    if (root_entries) *root_entries = h->ov.hash_cap;
    if (child_nodes) *child_nodes = h->ov.nodes_cap - h->ov.hash_cap;
    if (blocks) *blocks = h->ov.blocks_cap;
    return LK_OK;
}
}  // extern "C"
