// lk_c2c.hip - the map-cloud metric unit of liblegkilo_hip.so (see lk_internal.h): cloud-to-cloud nearest-neighbour distance of many pairs of clouds
// in one call (lk_c2c_kernels.h, arithmetic in lk_c2c.h) and the two C-ABI entries around it - lk_clouds_c2c_dev over clouds in HBM (a run replay's
// d_world_out, lk_downsample_clouds_dev's d_out), lk_clouds_c2c over clouds in host memory - and, on the same search structure (c2c_index), the
// scores that need no reference: mean map entropy and mean plane variance (lk_mme_kernels.h, arithmetic in lk_mme.h), lk_clouds_mme_dev / lk_clouds_mme,
// and the rigid alignment of a query cloud to its reference (lk_align_kernels.h, arithmetic in lk_align.h): lk_clouds_align_dev / lk_clouds_align run
// c2c_run's call with the search iterated under a transform, lk_clouds_transform_dev writes the moved clouds; lk_clouds_align_plane_dev /
// lk_clouds_align_plane are the same loop with the point-to-plane solve between the searches (lk_align_plane_kernels.h, arithmetic in
// lk_align_plane.h) against per-point normals of the reference, which lk_clouds_normals_dev / lk_clouds_normals make from MME's neighbourhood walk
// (lk_normals_kernels.h, arithmetic in lk_normals.h); lk_clouds_sor_dev / lk_clouds_sor remove a cloud's outliers by the mean distance to the k nearest
// neighbours (lk_sor_kernels.h, arithmetic in lk_sor.h) and write the kept records as clouds every entry above takes; lk_clouds_cluster_dev /
// lk_clouds_cluster label a cloud's points by DBSCAN cluster - connected components for min_pts 1 - and write the points of the clusters whose size
// is in bounds the same way (lk_cluster_kernels.h, arithmetic and the union-find in lk_cluster.h); lk_clouds_planes_dev / lk_clouds_planes peel the
// dominant planes off a cloud by RANSAC - no cell index, hypotheses x records - and write the remainder or the planes' points the same way
// (lk_planes_kernels.h, arithmetic in lk_planes.h).
// What the families share is written once.  Every neighbourhood is lk_c2c.h's ONE walk of the 27 cells with the family's visitor.  On the host:
// c2c_offsets_check / c2c_overlap_check and, for the single-cloud families, clouds_check_args / clouds_check_table (refusals, in MME's order);
// c2c_bounds (bounds and status of one side's clouds in use); c2c_carve and C2cIndex::take (the layout of a call in h->c2c and the index's tables in
// it); nonempty_clouds; c2c_or_own (the caller's per-point array or one of ours); scan_reserve and C2cTail (the compaction tail of the families that
// write kept records out: scan, output offsets, scatter); C2cStage (the host entries' trip through c2c_io).
// Two host round trips per call: none before the sort (the grids are built where the bounds lie), one at the end for the records.
#define LK_TU_C2C 1
#include "lk_internal.h"
#include "lk_c2c_kernels.h"
#include "lk_align_kernels.h"
#include "lk_align_plane_kernels.h"
#include "lk_mme_kernels.h"
#include "lk_normals_kernels.h"
#include "lk_sor_kernels.h"
#include "lk_cluster_kernels.h"
#include "lk_planes_kernels.h"

static_assert(sizeof(lk_c2c) == 80, "lk_c2c must be 80 B");
static_assert(sizeof(lk_mme) == 64, "lk_mme must be 64 B");
static_assert(sizeof(lk_align) == 136, "lk_align must be 136 B");
static_assert(sizeof(lk_align_plane) == 32, "lk_align_plane must be 32 B");
static_assert(sizeof(lk_normals) == 24, "lk_normals must be 24 B");
static_assert(sizeof(lk_sor) == 64, "lk_sor must be 64 B");
static_assert(sizeof(lk_cluster) == 64, "lk_cluster must be 64 B");
static_assert(sizeof(lk_planes) == 64 && sizeof(lk_plane) == 96, "lk_planes must be 64 B, lk_plane 96 B");
static_assert(LK_PLANES_HYP_LIMIT == LK_PLANES_MAX_HYP && LK_PLANES_CHUNK % LK_PLANES_TILE == 0, "lk_planes.h lays the sampler's counter out by LK_PLANES_MAX_HYP");
static_assert(sizeof(LkC2cRec) == 16 && sizeof(LkC2cGrid) == 40, "a reference record in cell order is 16 B, a grid 40 B");

namespace {
struct C2cArgs {   // the arguments both entries share, as the caller gave them
    const float *query, *ref;
    size_t n_q, n_r, n_pairs;
    const uint64_t *q_off, *r_off;
    const uint32_t *pair_q, *pair_r;
    double max_dist;
    const double* thr;
    uint32_t n_thr;
    lk_c2c* out;
    uint32_t* nn_idx;
    double* nn_d2;
    uint64_t* nn_off;
};
struct AlignArgs {   // what lk_clouds_align(_dev) adds to them (C2cArgs::out is then c2c_out, which may be null)
    const double* T0;
    uint32_t max_iter;
    double eps_rot, eps_trans;
    lk_align* out;
    const float* ref_normals;   // lk_clouds_align_plane(_dev) only (DEVICE in c2c_run): the solve between two searches is then the point-to-plane one
    lk_align_plane* pl_out;     // may be null
};
struct C2cSpan {   // a named range of bytes (p = 0: not given)
    const char* name;
    uintptr_t p;
    size_t len;
};
bool overlaps(const C2cSpan& a, const C2cSpan& b) { return a.len && b.len && a.p < b.p + b.len && b.p < a.p + a.len; }
}  // namespace

// an offset table does not decrease
static int c2c_offsets_check(lk_handle* h, const std::string& w, const char* name, const uint64_t* off, size_t n) {
    for (size_t c = 0; c < n; ++c)
        if (off[c + 1] < off[c]) return fail(h, LK_ERR_INVALID, w + name + " decreases at cloud " + std::to_string(c));
    return LK_OK;
}
// one named output against the input ranges (reported as `in_what`), then against the outputs in `rest`
static int c2c_overlap_check(lk_handle* h, const std::string& w, const C2cSpan& o, const C2cSpan* in, size_t n_in, const char* in_what, const C2cSpan* rest, size_t n_rest) {
    if (!o.p) return LK_OK;
    for (size_t k = 0; k < n_in; ++k)
        if (overlaps(o, in[k])) return fail(h, LK_ERR_INVALID, w + o.name + " overlaps " + in_what);
    for (size_t k = 0; k < n_rest; ++k)
        if (rest[k].p && overlaps(o, rest[k])) return fail(h, LK_ERR_INVALID, w + o.name + " overlaps " + rest[k].name);
    return LK_OK;
}
// in a carve: the caller's array, or `total` elements of our own
template <typename T>
static T* c2c_or_own(LkCarve& c, T* given, size_t total) {
    T* own = c.take<T>(given ? 0 : total);
    return given ? given : own;
}

// what both entries refuse before anything is launched; cloud_align: 16 for device clouds, 4 for host ones.  *total: query points over all pairs
static int c2c_check(lk_handle* h, const char* who, const C2cArgs& a, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    if (a.n_pairs == 0) return fail(h, LK_ERR_INVALID, w + "n_pairs is 0");
    if (!a.query) return fail(h, LK_ERR_INVALID, w + "null argument (query)");
    if (!a.ref) return fail(h, LK_ERR_INVALID, w + "null argument (ref)");
    if (!a.q_off) return fail(h, LK_ERR_INVALID, w + "null argument (q_off)");
    if (!a.r_off) return fail(h, LK_ERR_INVALID, w + "null argument (r_off)");
    if (!a.pair_q) return fail(h, LK_ERR_INVALID, w + "null argument (pair_q)");
    if (!a.pair_r) return fail(h, LK_ERR_INVALID, w + "null argument (pair_r)");
    if (!a.out) return fail(h, LK_ERR_INVALID, w + "null argument (out)");
    if (!a.nn_idx != !a.nn_d2) return fail(h, LK_ERR_INVALID, w + (a.nn_idx ? "nn_idx without nn_d2" : "nn_d2 without nn_idx") + ": both or neither");
    if (a.nn_idx && !a.nn_off) return fail(h, LK_ERR_INVALID, w + "nn_idx and nn_d2 need nn_off");
    if ((uintptr_t)a.query & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "query must be " + std::to_string(cloud_align) + "-byte aligned");
    if ((uintptr_t)a.ref & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "ref must be " + std::to_string(cloud_align) + "-byte aligned");
    if ((uintptr_t)a.nn_idx & 3) return fail(h, LK_ERR_INVALID, w + "nn_idx must be 4-byte aligned");
    if ((uintptr_t)a.nn_d2 & 7) return fail(h, LK_ERR_INVALID, w + "nn_d2 must be 8-byte aligned");
    if (!std::isfinite(a.max_dist) || !(a.max_dist > 0.0)) return fail(h, LK_ERR_INVALID, w + "max_dist must be finite and above 0");
    if (a.n_thr > 4) return fail(h, LK_ERR_INVALID, w + "n_thr is " + std::to_string(a.n_thr) + ": at most 4 thresholds");
    if (a.n_thr && !a.thr) return fail(h, LK_ERR_INVALID, w + "null argument (thr) with n_thr above 0");
    for (uint32_t k = 0; k < a.n_thr; ++k)
        if (!std::isfinite(a.thr[k]) || a.thr[k] < 0.0 || a.thr[k] > a.max_dist)
            return fail(h, LK_ERR_INVALID, w + "thr[" + std::to_string(k) + "] must be finite and in 0 .. max_dist");
    LKCHK(c2c_offsets_check(h, w, "q_off", a.q_off, a.n_q));
    LKCHK(c2c_offsets_check(h, w, "r_off", a.r_off, a.n_r));
    for (size_t k = 0; k < a.n_pairs; ++k) {
        if (a.pair_q[k] >= a.n_q) return fail(h, LK_ERR_INVALID, w + "pair_q[" + std::to_string(k) + "] is past the " + std::to_string(a.n_q) + " query clouds");
        if (a.pair_r[k] >= a.n_r) return fail(h, LK_ERR_INVALID, w + "pair_r[" + std::to_string(k) + "] is past the " + std::to_string(a.n_r) + " reference clouds");
    }
    // (pairs exist, so both sides hold a cloud and both tables an entry 0)
    if (a.n_pairs >= 0xffffffffull || a.n_q >= 0xffffffffull || a.n_r >= 0x7fffffffull) return fail(h, LK_ERR_CAPACITY, w + "2^32 - 1 pairs or clouds or more");
    if (a.r_off[a.n_r] - a.r_off[0] >= (1ull << 31)) return fail(h, LK_ERR_CAPACITY, w + "ref holds 2^31 records or more in all: split the call");
    unsigned long long sum = 0;
    for (size_t k = 0; k < a.n_pairs; ++k) {
        const uint64_t n = a.q_off[a.pair_q[k] + 1] - a.q_off[a.pair_q[k]];
        if (n >= 0xffffffffull) return fail(h, LK_ERR_CAPACITY, w + "query cloud " + std::to_string(a.pair_q[k]) + " holds 2^32 - 1 records or more");
        sum += n;
        if (sum >= (1ull << 32)) return fail(h, LK_ERR_CAPACITY, w + "the pairs' query clouds hold 2^32 records or more in all: split the call");
    }
    *total = (size_t)sum;
    const C2cSpan in[2] = {{"query", (uintptr_t)a.query + 16u * (uintptr_t)a.q_off[0], 16u * (size_t)(a.q_off[a.n_q] - a.q_off[0])},
                           {"ref", (uintptr_t)a.ref + 16u * (uintptr_t)a.r_off[0], 16u * (size_t)(a.r_off[a.n_r] - a.r_off[0])}};
    const C2cSpan idx = {"nn_idx", (uintptr_t)a.nn_idx, 4 * *total}, d2 = {"nn_d2", (uintptr_t)a.nn_d2, 8 * *total};
    LKCHK(c2c_overlap_check(h, w, idx, in, 2, "an input cloud", nullptr, 0));
    LKCHK(c2c_overlap_check(h, w, d2, in, 2, "an input cloud", nullptr, 0));
    return c2c_overlap_check(h, w, idx, nullptr, 0, "", &d2, 1);
}

// the clouds of one side that a pair names, in ascending order
static std::vector<unsigned int> used_clouds(const uint32_t* pair, size_t n_pairs, size_t n_clouds) {
    std::vector<unsigned char> seen(n_clouds, 0);
    for (size_t k = 0; k < n_pairs; ++k) seen[pair[k]] = 1;
    std::vector<unsigned int> u;
    for (size_t c = 0; c < n_clouds; ++c)
        if (seen[c]) u.push_back((unsigned int)c);
    return u;
}

// The search structure of one side's clouds (steps 1 and 2 of a call), shared by every family that walks cells: the device tables, which take() carves
// out of the caller's layout for n clouds, n_used of them in use, N = off[n] - off[0] records in all.
struct C2cIndex {
    unsigned long long* d_off64;   // [n + 1], as given
    unsigned int* d_off;           // [n + 1], counted from the first record
    unsigned int* d_used;          // [used.size()]
    unsigned int* status;          // [n]
    int* mm;                       // [6 n]
    LkC2cGrid* grid;               // [n]
    unsigned int *k0, *k1, *v0, *v1;   // [N]: k1 = the sorted keys
    LkC2cRec* recs;                // [N], in that order
    std::vector<unsigned int> h_off;   // the host copy of d_off: alive until the caller has synchronised
    void take(LkCarve& c, size_t n, size_t n_used, size_t N) {
        d_off64 = c.take<unsigned long long>(n + 1), d_off = c.take<unsigned int>(n + 1), d_used = c.take<unsigned int>(n_used);
        status = c.take<unsigned int>(n), mm = c.take<int>(6 * n), grid = c.take<LkC2cGrid>(n);
        k0 = c.take<unsigned int>(N), k1 = c.take<unsigned int>(N), v0 = c.take<unsigned int>(N), v1 = c.take<unsigned int>(N);
        recs = c.take<LkC2cRec>(N);
    }
};
// every non-empty cloud: what the single-cloud families have in use
static std::vector<unsigned int> nonempty_clouds(const uint64_t* off, size_t n) {
    std::vector<unsigned int> used;
    for (size_t c = 0; c < n; ++c)
        if (off[c + 1] > off[c]) used.push_back((unsigned int)c);
    return used;
}
// a layout (lk_carve.h) over h->c2c: counted, reserved with a quarter of slack, then handed out
template <class F>
static int c2c_carve(lk_handle* h, F&& layout) {
    LkCarve count(nullptr, 256);
    layout(count);
    LKCHK(reserve(h, h->c2c, count.total(), count.total() / 4));
    LkCarve c(h->c2c.p, 256);
    layout(c);
    return LK_OK;
}
static dim3 c2c_blocks(size_t n) { return dim3((unsigned int)((n + 255) / 256)); }
static int c2c_sort(lk_handle* h, void* tmp, size_t& tb, const C2cIndex& x, size_t N, size_t n) {
    HIPCHK(h, lk_prim_sort_pairs_in_segments(tmp, tb, x.k0, x.k1, x.v0, x.v1, (unsigned int)N, (unsigned int)n, x.d_off, x.d_off + 1, 0, 31, h->stream));
    return LK_OK;
}
// bounds and status of one side's clouds in use (d_off64, d_used: the device copies of off and used, already on their way)
static int c2c_bounds(lk_handle* h, const float4* pts, const uint64_t* off, size_t n, const std::vector<unsigned int>& used, const unsigned long long* d_off64,
                      const unsigned int* d_used, double reach, int* mm, unsigned int* status) {
    size_t big = 0;
    for (unsigned int c : used) big = std::max(big, (size_t)(off[c + 1] - off[c]));
    LAUNCH(h, "c2c_init", hipLaunchKernelGGL(lk_c2c_init_kernel, c2c_blocks(n), dim3(256), 0, h->stream, mm, status, (unsigned int)n));
    if (!used.empty())
        LAUNCH(h, "c2c_bounds", hipLaunchKernelGGL(lk_c2c_bounds_kernel, dim3((unsigned int)used.size(), bounds_rows(used.size(), big)), dim3(256), 0, h->stream,
                                                   pts, d_off64, d_used, reach, mm, status));
    return LK_OK;
}
// 1. bounds and status of the clouds in use (c2c_bounds) and every cloud's grid at edge `reach` (doubling as lk_c2c_grid says); 2. a cell key per record, a stable
// sort by key inside each cloud, the records into that order
static int c2c_index(lk_handle* h, const float4* pts, const uint64_t* off, size_t n, const std::vector<unsigned int>& used, double reach, C2cIndex& x) {
    const size_t N = (size_t)(off[n] - off[0]);
    if (N) {
        size_t tb = 0;
        LKCHK(c2c_sort(h, nullptr, tb, x, N, n));
        LKCHK(reserve(h, h->prim_tmp, tb));
    }
    std::vector<unsigned int>& roff = x.h_off;
    roff.resize(n + 1);
    for (size_t c = 0; c <= n; ++c) roff[c] = (unsigned int)(off[c] - off[0]);
    HIPCHK(h, hipMemcpyAsync(x.d_off64, off, 8 * (n + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(x.d_off, roff.data(), 4 * (n + 1), hipMemcpyHostToDevice, h->stream));
    if (!used.empty()) HIPCHK(h, hipMemcpyAsync(x.d_used, used.data(), 4 * used.size(), hipMemcpyHostToDevice, h->stream));
    LKCHK(c2c_bounds(h, pts, off, n, used, x.d_off64, x.d_used, reach, x.mm, x.status));
    LAUNCH(h, "c2c_grid", hipLaunchKernelGGL(lk_c2c_grid_kernel, c2c_blocks(n), dim3(256), 0, h->stream, x.mm, x.status, reach, (unsigned int)n, x.grid));
    if (N) {
        const float4* first = pts + off[0];
        LAUNCH(h, "c2c_keys", hipLaunchKernelGGL(lk_c2c_keys_kernel, c2c_blocks(N), dim3(256), 0, h->stream, first, (unsigned int)N, x.d_off, (unsigned int)n, x.grid,
                                                 x.status, x.mm, x.k0, x.v0));
        size_t tb = h->prim_tmp.cap;
        LKCHK(c2c_sort(h, h->prim_tmp.p, tb, x, N, n));
        LAUNCH(h, "c2c_gather", hipLaunchKernelGGL(lk_c2c_gather_kernel, c2c_blocks(N), dim3(256), 0, h->stream, first, x.v1, (unsigned int)N, x.d_off, (unsigned int)n,
                                                   x.status, x.mm, x.recs));
    }
    return LK_OK;
}

// the call behind c2c_check, on DEVICE clouds and DEVICE nn arrays (null: the library's own).  al: the alignment's arguments - step 3 is then the
// loop of lk_align_kernels.h, enqueued back to back: max_iter + 1 searches with max_iter solves between them, and the same final reduce
static int c2c_run(lk_handle* h, const C2cArgs& a, size_t total, const AlignArgs* al = nullptr) {
    const size_t NQ = a.n_q, NR = a.n_r, P = a.n_pairs, N = (size_t)(a.r_off[NR] - a.r_off[0]);
    const std::vector<unsigned int> uq = used_clouds(a.pair_q, P, NQ), ur = used_clouds(a.pair_r, P, NR);
    LkC2cQuery q = {};
    C2cIndex x = {};
    unsigned long long *d_qoff = nullptr, *d_nnoff = nullptr;
    unsigned int *d_pq = nullptr, *d_pr = nullptr, *d_uq = nullptr, *q_status = nullptr;
    int* q_mm = nullptr;
    LkAlignCall call = {};
    double* d_T0 = nullptr;
    lk_align_plane* d_pl = nullptr;
    const bool plane = al && al->ref_normals;
    LKCHK(c2c_carve(h, [&](LkCarve& c) {
        x.take(c, NR, ur.size(), N);
        d_qoff = c.take<unsigned long long>(NQ + 1), d_nnoff = c.take<unsigned long long>(P + 1);
        d_pq = c.take<unsigned int>(P), d_pr = c.take<unsigned int>(P), d_uq = c.take<unsigned int>(uq.size());
        q_status = c.take<unsigned int>(NQ), q_mm = c.take<int>(6 * NQ);
        q.nn_idx = c2c_or_own(c, a.nn_idx, total), q.nn_d2 = c2c_or_own(c, a.nn_d2, total);   // (c2c_check: both or neither)
        q.out = c.take<lk_c2c>(P);
        d_T0 = c.take<double>(al ? 12 * P : 0), call.rec = c.take<lk_align>(al ? P : 0), call.done = c.take<unsigned int>(al ? P : 0);
        d_pl = c.take<lk_align_plane>(plane ? P : 0);
    }));
    // the host tables of the query side and of the pairs
    std::vector<unsigned long long> nnoff(P + 1, 0ull);
    for (size_t k = 0; k < P; ++k) nnoff[k + 1] = nnoff[k] + (a.q_off[a.pair_q[k] + 1] - a.q_off[a.pair_q[k]]);
    HIPCHK(h, hipMemcpyAsync(d_qoff, a.q_off, 8 * (NQ + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_nnoff, nnoff.data(), 8 * (P + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_pq, a.pair_q, 4 * P, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_pr, a.pair_r, 4 * P, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_uq, uq.data(), 4 * uq.size(), hipMemcpyHostToDevice, h->stream));
    const float4* qpts = reinterpret_cast<const float4*>(a.query);
    const float4* rpts = reinterpret_cast<const float4*>(a.ref);
    // bounds and status of the query clouds in use; steps 1 and 2 for the reference side
    LKCHK(c2c_bounds(h, qpts, a.q_off, NQ, uq, d_qoff, d_uq, a.max_dist, q_mm, q_status));
    LKCHK(c2c_index(h, rpts, a.r_off, NR, ur, a.max_dist, x));
    // 3. (j, d2) per pair and query point, one record per pair
    q.q_pts = qpts, q.q_off = d_qoff, q.r_off = x.d_off, q.pair_q = d_pq, q.pair_r = d_pr, q.nn_off = d_nnoff;
    q.q_status = q_status, q.r_status = x.status, q.grid = x.grid, q.keys = x.k1, q.recs = x.recs;
    q.reach2 = lk_c2c_reach2(a.max_dist);
    for (uint32_t k = 0; k < 4; ++k) q.thr2[k] = k < a.n_thr ? a.thr[k] * a.thr[k] : 0.0;
    q.n_pairs = (unsigned int)P, q.n_thr = a.n_thr;
    std::vector<double> t0;          // alive until the stream has been synchronised
    std::vector<lk_align> arec;
    std::vector<lk_align_plane> prec;
    if (!al) {
        if (total) LAUNCH(h, "c2c_query", hipLaunchKernelGGL(lk_c2c_query_kernel, c2c_blocks(total), dim3(256), 0, h->stream, q, (unsigned long long)total));
    } else {
        t0.resize(12 * P);
        for (size_t k = 0; k < P; ++k)
            for (int i = 0; i < 12; ++i) t0[12 * k + i] = al->T0 ? al->T0[12 * k + i] : ((i == 0 || i == 4 || i == 8) ? 1.0 : 0.0);
        HIPCHK(h, hipMemcpyAsync(d_T0, t0.data(), 8 * t0.size(), hipMemcpyHostToDevice, h->stream));
        call.q = q, call.r_pts = rpts, call.r_off64 = x.d_off64, call.T0 = d_T0;
        call.max_dist = a.max_dist, call.eps_rot = al->eps_rot, call.eps_trans = al->eps_trans;
        LAUNCH(h, "align_init", hipLaunchKernelGGL(lk_align_init_kernel, c2c_blocks(P), dim3(256), 0, h->stream, call));
        for (uint32_t it = 0; it <= al->max_iter; ++it) {
            if (total)
                LAUNCH(h, "align_search", hipLaunchKernelGGL(lk_align_search_kernel, c2c_blocks(total), dim3(256), 0, h->stream, call, (unsigned long long)total, it == 0 ? 1 : 0));
            if (plane)   // (also after the last search: every pair's final search gets its plane figures there)
                LAUNCH(h, "align_plane_solve", hipLaunchKernelGGL(lk_align_plane_solve_kernel, dim3((unsigned int)P), dim3(256), 0, h->stream, call,
                                                                  reinterpret_cast<const float4*>(al->ref_normals), d_pl, it == 0 ? 1 : 0, it == al->max_iter ? 1 : 0));
            else if (it < al->max_iter) LAUNCH(h, "align_solve", hipLaunchKernelGGL(lk_align_solve_kernel, dim3((unsigned int)P), dim3(256), 0, h->stream, call));
        }
    }
    LAUNCH(h, "c2c_reduce", hipLaunchKernelGGL(lk_c2c_reduce_kernel, dim3((unsigned int)P), dim3(256), 0, h->stream, q));
    std::vector<lk_c2c> rec(P);
    HIPCHK(h, hipMemcpyAsync(rec.data(), q.out, sizeof(lk_c2c) * P, hipMemcpyDeviceToHost, h->stream));
    if (al) {
        if (al->max_iter == 0 && !plane) LAUNCH(h, "align_first_is_last", hipLaunchKernelGGL(lk_align_first_is_last_kernel, c2c_blocks(P), dim3(256), 0, h->stream, call));
        arec.resize(P);
        HIPCHK(h, hipMemcpyAsync(arec.data(), call.rec, sizeof(lk_align) * P, hipMemcpyDeviceToHost, h->stream));
        if (plane && al->pl_out) {
            prec.resize(P);
            HIPCHK(h, hipMemcpyAsync(prec.data(), d_pl, sizeof(lk_align_plane) * P, hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (a.out) memcpy(a.out, rec.data(), sizeof(lk_c2c) * P);
    if (al) memcpy(al->out, arec.data(), sizeof(lk_align) * P);
    if (!prec.empty()) memcpy(al->pl_out, prec.data(), sizeof(lk_align_plane) * P);
    if (a.nn_off)
        for (size_t k = 0; k <= P; ++k) a.nn_off[k] = nnoff[k];
    return LK_OK;
}

// The host entries' trip through c2c_io: every range of host records and every host per-point array that was asked for gets a device twin (+ 1 element:
// an empty one still has an address of its own); the records go up, their offsets are rebased to each range's first record; after the run fetch()
// copies the arrays back and synchronises once
namespace {
struct C2cStage {
    struct In {   // rel = off - off[0]
        const float* host; const uint64_t* off; size_t n_clouds; float4* dev; std::vector<uint64_t> rel;
        const float* f() const { return reinterpret_cast<const float*>(dev); }
    };
    struct Out {   // host null: not asked for, dev null
        void* host; size_t elem, count; void* dev;
        template <typename T> operator T*() const { return static_cast<T*>(dev); }   // the device twin as the array it stands for
    };
    std::vector<In> in;
    std::vector<Out> out;
    // the pair families: the query and the reference clouds (and what else lies along the reference records), nn_idx and nn_d2; `a` then names the twins
    int upload_pairs(lk_handle* h, C2cArgs& a, size_t total, const float** along_ref = nullptr) {
        in = {{a.query, a.q_off, a.n_q}, {a.ref, a.r_off, a.n_r}};
        if (along_ref) in.push_back({*along_ref, a.r_off, a.n_r});
        out = {{a.nn_idx, 4, total}, {a.nn_idx ? a.nn_d2 : nullptr, 8, total}};
        LKCHK(upload(h));
        a.query = in[0].f(), a.ref = in[1].f(), a.q_off = in[0].rel.data(), a.r_off = in[1].rel.data();
        a.nn_idx = out[0], a.nn_d2 = out[1];
        if (along_ref) *along_ref = in[2].f();
        return LK_OK;
    }
    // the single-cloud families: the clouds; the caller lists `out`
    int upload_clouds(lk_handle* h, const float*& clouds, size_t n_clouds, const uint64_t*& off) {
        in = {{clouds, off, n_clouds}};
        LKCHK(upload(h));
        clouds = in[0].f(), off = in[0].rel.data();
        return LK_OK;
    }
    int upload(lk_handle* h) {
        auto carve = [&](void* base) {
            LkCarve c(base, 256);
            for (In& i : in) i.dev = c.take<float4>((size_t)(i.off[i.n_clouds] - i.off[0]) + 1);
            for (Out& o : out) o.dev = o.host ? c.take<unsigned char>(o.elem * (o.count + 1)) : nullptr;
            return c.total();
        };
        LKCHK(reserve(h, h->c2c_io, carve(nullptr)));
        carve(h->c2c_io.p);
        for (In& i : in) {
            const size_t n = (size_t)(i.off[i.n_clouds] - i.off[0]);
            if (n) HIPCHK(h, hipMemcpyAsync(i.dev, i.host + 4 * i.off[0], 16 * n, hipMemcpyHostToDevice, h->stream));
            for (size_t c = 0; c <= i.n_clouds; ++c) i.rel.push_back(i.off[c] - i.off[0]);
        }
        return LK_OK;
    }
    int fetch(lk_handle* h) {
        bool any = false;
        for (const Out& o : out) {
            if (!o.host || !o.count) continue;
            HIPCHK(h, hipMemcpyAsync(o.host, o.dev, o.elem * o.count, hipMemcpyDeviceToHost, h->stream));
            any = true;
        }
        if (any) HIPCHK(h, hipStreamSynchronize(h->stream));
        return LK_OK;
    }
};
}  // namespace

extern "C" {

int lk_clouds_c2c_dev(lk_handle* h, const float* d_query, size_t n_qclouds, const uint64_t* q_off, const float* d_ref, size_t n_rclouds, const uint64_t* r_off,
                      size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r, double max_dist, const double* thr, uint32_t n_thr, lk_c2c* out,
                      uint32_t* d_nn_idx, double* d_nn_d2, uint64_t* nn_off) {
    CHECK_H(h);
    const C2cArgs a = {d_query, d_ref, n_qclouds, n_rclouds, n_pairs, q_off, r_off, pair_q, pair_r, max_dist, thr, n_thr, out, d_nn_idx, d_nn_d2, nn_off};
    size_t total = 0;
    LKCHK(c2c_check(h, "lk_clouds_c2c_dev", a, 16, &total));
    return c2c_run(h, a, total);
}

int lk_clouds_c2c(lk_handle* h, const float* query, size_t n_qclouds, const uint64_t* q_off, const float* ref, size_t n_rclouds, const uint64_t* r_off,
                  size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r, double max_dist, const double* thr, uint32_t n_thr, lk_c2c* out, uint32_t* nn_idx,
                  double* nn_d2, uint64_t* nn_off) {
    CHECK_H(h);
    C2cArgs a = {query, ref, n_qclouds, n_rclouds, n_pairs, q_off, r_off, pair_q, pair_r, max_dist, thr, n_thr, out, nn_idx, nn_d2, nn_off};
    size_t total = 0;
    LKCHK(c2c_check(h, "lk_clouds_c2c", a, 4, &total));
    C2cStage st;
    LKCHK(st.upload_pairs(h, a, total));
    LKCHK(c2c_run(h, a, total));
    return st.fetch(h);
}

// what lk_clouds_align(_dev) refuses: every refusal of the C2C entry of the same memory, then its own arguments
static int align_check(lk_handle* h, const char* who, const C2cArgs& a, const AlignArgs& al, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    lk_c2c sink;
    C2cArgs c = a;
    c.out = &sink;   // (c2c_out is optional here; `out` is checked below)
    LKCHK(c2c_check(h, who, c, cloud_align, total));
    if (!al.out) return fail(h, LK_ERR_INVALID, w + "null argument (out)");
    if (al.max_iter > 1000u) return fail(h, LK_ERR_INVALID, w + "max_iter is " + std::to_string(al.max_iter) + ": at most 1000");
    if (!std::isfinite(al.eps_rot) || al.eps_rot < 0.0) return fail(h, LK_ERR_INVALID, w + "eps_rot must be finite and at least 0");
    if (!std::isfinite(al.eps_trans) || al.eps_trans < 0.0) return fail(h, LK_ERR_INVALID, w + "eps_trans must be finite and at least 0");
    return LK_OK;
}

int lk_clouds_align_dev(lk_handle* h, const float* d_query, size_t n_qclouds, const uint64_t* q_off, const float* d_ref, size_t n_rclouds, const uint64_t* r_off,
                        size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r, double max_dist, const double* thr, uint32_t n_thr, const double* T0,
                        uint32_t max_iter, double eps_rot, double eps_trans, lk_align* out, lk_c2c* c2c_out, uint32_t* d_nn_idx, double* d_nn_d2, uint64_t* nn_off) {
    CHECK_H(h);
    const C2cArgs a = {d_query, d_ref, n_qclouds, n_rclouds, n_pairs, q_off, r_off, pair_q, pair_r, max_dist, thr, n_thr, c2c_out, d_nn_idx, d_nn_d2, nn_off};
    const AlignArgs al = {T0, max_iter, eps_rot, eps_trans, out};
    size_t total = 0;
    LKCHK(align_check(h, "lk_clouds_align_dev", a, al, 16, &total));
    return c2c_run(h, a, total, &al);
}

int lk_clouds_align(lk_handle* h, const float* query, size_t n_qclouds, const uint64_t* q_off, const float* ref, size_t n_rclouds, const uint64_t* r_off,
                    size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r, double max_dist, const double* thr, uint32_t n_thr, const double* T0,
                    uint32_t max_iter, double eps_rot, double eps_trans, lk_align* out, lk_c2c* c2c_out, uint32_t* nn_idx, double* nn_d2, uint64_t* nn_off) {
    CHECK_H(h);
    C2cArgs a = {query, ref, n_qclouds, n_rclouds, n_pairs, q_off, r_off, pair_q, pair_r, max_dist, thr, n_thr, c2c_out, nn_idx, nn_d2, nn_off};
    const AlignArgs al = {T0, max_iter, eps_rot, eps_trans, out};
    size_t total = 0;
    LKCHK(align_check(h, "lk_clouds_align", a, al, 4, &total));
    C2cStage st;
    LKCHK(st.upload_pairs(h, a, total));
    LKCHK(c2c_run(h, a, total, &al));
    return st.fetch(h);
}

// what lk_clouds_align_plane(_dev) refuses: every refusal of the alignment entry of the same memory, then the normals
static int align_plane_check(lk_handle* h, const char* who, const C2cArgs& a, const AlignArgs& al, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    LKCHK(align_check(h, who, a, al, cloud_align, total));
    if (!al.ref_normals) return fail(h, LK_ERR_INVALID, w + "null argument (ref_normals)");
    if ((uintptr_t)al.ref_normals & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "ref_normals must be " + std::to_string(cloud_align) + "-byte aligned");
    const C2cSpan nrm = {"ref_normals", (uintptr_t)al.ref_normals + 16u * (uintptr_t)a.r_off[0], 16u * (size_t)(a.r_off[a.n_r] - a.r_off[0])};
    const C2cSpan idx = {"nn_idx", (uintptr_t)a.nn_idx, 4 * *total}, d2 = {"nn_d2", (uintptr_t)a.nn_d2, 8 * *total};
    LKCHK(c2c_overlap_check(h, w, idx, &nrm, 1, "ref_normals", nullptr, 0));
    return c2c_overlap_check(h, w, d2, &nrm, 1, "ref_normals", nullptr, 0);
}

int lk_clouds_align_plane_dev(lk_handle* h, const float* d_query, size_t n_qclouds, const uint64_t* q_off, const float* d_ref, size_t n_rclouds, const uint64_t* r_off,
                              size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r, double max_dist, const double* thr, uint32_t n_thr, const double* T0,
                              uint32_t max_iter, double eps_rot, double eps_trans, const float* d_ref_normals, lk_align* out, lk_align_plane* pl_out, lk_c2c* c2c_out,
                              uint32_t* d_nn_idx, double* d_nn_d2, uint64_t* nn_off) {
    CHECK_H(h);
    const C2cArgs a = {d_query, d_ref, n_qclouds, n_rclouds, n_pairs, q_off, r_off, pair_q, pair_r, max_dist, thr, n_thr, c2c_out, d_nn_idx, d_nn_d2, nn_off};
    const AlignArgs al = {T0, max_iter, eps_rot, eps_trans, out, d_ref_normals, pl_out};
    size_t total = 0;
    LKCHK(align_plane_check(h, "lk_clouds_align_plane_dev", a, al, 16, &total));
    return c2c_run(h, a, total, &al);
}

int lk_clouds_align_plane(lk_handle* h, const float* query, size_t n_qclouds, const uint64_t* q_off, const float* ref, size_t n_rclouds, const uint64_t* r_off,
                          size_t n_pairs, const uint32_t* pair_q, const uint32_t* pair_r, double max_dist, const double* thr, uint32_t n_thr, const double* T0,
                          uint32_t max_iter, double eps_rot, double eps_trans, const float* ref_normals, lk_align* out, lk_align_plane* pl_out, lk_c2c* c2c_out,
                          uint32_t* nn_idx, double* nn_d2, uint64_t* nn_off) {
    CHECK_H(h);
    C2cArgs a = {query, ref, n_qclouds, n_rclouds, n_pairs, q_off, r_off, pair_q, pair_r, max_dist, thr, n_thr, c2c_out, nn_idx, nn_d2, nn_off};
    AlignArgs al = {T0, max_iter, eps_rot, eps_trans, out, ref_normals, pl_out};
    size_t total = 0;
    LKCHK(align_plane_check(h, "lk_clouds_align_plane", a, al, 4, &total));
    C2cStage st;
    LKCHK(st.upload_pairs(h, a, total, &al.ref_normals));
    LKCHK(c2c_run(h, a, total, &al));
    return st.fetch(h);
}

int lk_clouds_transform_dev(lk_handle* h, const float* d_in, size_t n_clouds, const uint64_t* off, const double* T, float* d_out) {
    CHECK_H(h);
    const std::string w = "lk_clouds_transform_dev: ";
    if (n_clouds == 0) return fail(h, LK_ERR_INVALID, w + "n_clouds is 0");
    if (!d_in) return fail(h, LK_ERR_INVALID, w + "null argument (d_in)");
    if (!off) return fail(h, LK_ERR_INVALID, w + "null argument (off)");
    if (!T) return fail(h, LK_ERR_INVALID, w + "null argument (T)");
    if (!d_out) return fail(h, LK_ERR_INVALID, w + "null argument (d_out)");
    if ((uintptr_t)d_in & 15) return fail(h, LK_ERR_INVALID, w + "d_in must be 16-byte aligned");
    if ((uintptr_t)d_out & 15) return fail(h, LK_ERR_INVALID, w + "d_out must be 16-byte aligned");
    LKCHK(c2c_offsets_check(h, w, "off", off, n_clouds));
    for (size_t k = 0; k < 12 * n_clouds; ++k)
        if (!std::isfinite(T[k])) return fail(h, LK_ERR_INVALID, w + "T[" + std::to_string(k / 12) + "] holds a non-finite entry");
    const uint64_t N = off[n_clouds] - off[0];
    if (n_clouds >= 0xffffffffull || N >= (1ull << 32)) return fail(h, LK_ERR_CAPACITY, w + "2^32 records or clouds or more: split the call");
    const float* first = d_in + 4 * off[0];
    const C2cSpan in = {"d_in", (uintptr_t)first, 16u * (size_t)N}, out = {"d_out", (uintptr_t)d_out, 16u * (size_t)N};
    if (d_out != first && overlaps(in, out)) return fail(h, LK_ERR_INVALID, w + "d_out overlaps d_in (in place is d_out == d_in + 4 * off[0] exactly)");
    unsigned long long* d_rel = nullptr;
    double* d_T = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base, 256);
        d_rel = c.take<unsigned long long>(n_clouds + 1), d_T = c.take<double>(12 * n_clouds);
        return c.total();
    };
    LKCHK(reserve(h, h->c2c, carve(nullptr)));
    carve(h->c2c.p);
    std::vector<unsigned long long> rel(n_clouds + 1);
    for (size_t c = 0; c <= n_clouds; ++c) rel[c] = off[c] - off[0];
    HIPCHK(h, hipMemcpyAsync(d_rel, rel.data(), 8 * rel.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_T, T, 96 * n_clouds, hipMemcpyHostToDevice, h->stream));
    if (N)
        LAUNCH(h, "clouds_transform", hipLaunchKernelGGL(lk_clouds_transform_kernel, c2c_blocks((size_t)N), dim3(256), 0, h->stream, reinterpret_cast<const float4*>(first),
                                                         d_rel, (unsigned int)n_clouds, d_T, reinterpret_cast<float4*>(d_out), (unsigned long long)N));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LK_OK;
}

}  // extern "C"

namespace {
struct MmeArgs {   // the arguments both entries share, as the caller gave them
    const float* clouds;
    size_t n_clouds;
    const uint64_t* off;
    double radius;
    uint32_t min_pts;
    lk_mme* out;
    uint32_t* n;
    double *hh, *lmin;
};
}  // namespace

// What every single-cloud family refuses about its clouds, in two halves.  The order of refusals is lk_clouds_mme(_dev)'s, and a caller that passes
// several bad arguments is told about the first in it: (1) n_clouds 0; (2) clouds, off, out null, in that order; (3) clouds misaligned -
// clouds_check_args.  (4) the family's own per-point arrays misaligned, its radius, its min_pts - MME's and the normals' radius stand HERE, between
// the halves; the reach of the filter and of the clustering is refused in front of (1).  (5) off decreases; (6) 2^31 - 1 clouds; (7) 2^31 records
// in all; (8) 2^32 - 1 records in a cloud - clouds_check_table, which also sets *total: records in all.  (9) everything else of the family's own.
// cloud_align: 16 for device clouds, 4 for host ones.
static int clouds_check_args(lk_handle* h, const std::string& w, const float* clouds, size_t n_clouds, const uint64_t* off, const void* out, unsigned int cloud_align) {
    if (n_clouds == 0) return fail(h, LK_ERR_INVALID, w + "n_clouds is 0");
    if (!clouds) return fail(h, LK_ERR_INVALID, w + "null argument (clouds)");
    if (!off) return fail(h, LK_ERR_INVALID, w + "null argument (off)");
    if (!out) return fail(h, LK_ERR_INVALID, w + "null argument (out)");
    if ((uintptr_t)clouds & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "clouds must be " + std::to_string(cloud_align) + "-byte aligned");
    return LK_OK;
}
static int clouds_check_table(lk_handle* h, const std::string& w, size_t n_clouds, const uint64_t* off, size_t* total) {
    LKCHK(c2c_offsets_check(h, w, "off", off, n_clouds));
    if (n_clouds >= 0x7fffffffull) return fail(h, LK_ERR_CAPACITY, w + "2^31 - 1 clouds or more");
    if (off[n_clouds] - off[0] >= (1ull << 31)) return fail(h, LK_ERR_CAPACITY, w + "the clouds hold 2^31 records or more in all: split the call");
    for (size_t c = 0; c < n_clouds; ++c)   // (cannot happen under the bound above; the header states both)
        if (off[c + 1] - off[c] >= 0xffffffffull) return fail(h, LK_ERR_CAPACITY, w + "cloud " + std::to_string(c) + " holds 2^32 - 1 records or more");
    *total = (size_t)(off[n_clouds] - off[0]);
    return LK_OK;
}
static int radius_check(lk_handle* h, const std::string& w, const char* name, double r) {
    if (!std::isfinite(r) || !(r > 0.0)) return fail(h, LK_ERR_INVALID, w + name + " must be finite and above 0");
    return LK_OK;
}
// the scan's temporary storage for n words, before anything is launched: growing it waits for the stream
static int scan_reserve(lk_handle* h, const unsigned int* in, unsigned int* out, size_t n) {
    size_t tb = 0;
    HIPCHK(h, lk_prim_exclusive_scan(nullptr, tb, in, out, n, h->stream));
    return reserve(h, h->prim_tmp, tb);
}

// The compaction tail of the families that write their kept records out as clouds (outlier filter, clustering, plane extraction): each brings the
// keep words of its own flag kernel; the scan over them, the output offsets, their copy to the host and the scatter are enqueued here, and after the
// caller's synchronisation finish() fills the caller's out_off.  No out_off: no places were asked for, and nothing here does anything.
struct C2cTail {
    LkCompactCall c = {};
    uint64_t* out_off;                 // the caller's table
    bool moved;                        // out_cloud or src_idx asked for
    std::vector<unsigned int> h_off;   // the host copy of c.out_off: alive until the caller has synchronised
    C2cTail(const float* clouds, const uint64_t* off, float* out_cloud, uint64_t* out_off_, uint32_t* src_idx) : out_off(out_off_), moved(out_cloud || src_idx) {
        c.in = reinterpret_cast<const uint4*>(clouds) + off[0], c.out_pts = reinterpret_cast<uint4*>(out_cloud), c.src_idx = src_idx;
    }
    // out_off and the scan's array; a family that has one for scans of its own (own_scan false) points c.scan at it instead
    void take(LkCarve& cv, size_t NC, size_t N, bool own_scan = true) {
        if (own_scan) c.scan = cv.take<unsigned int>(out_off ? N + 1 : 0);
        c.out_off = cv.take<unsigned int>(out_off ? NC + 1 : 0);
    }
    // behind the family's flag kernel (the scan's temporary storage is reserved: scan_reserve).  d_off: the clouds' table from the first record
    int enqueue(lk_handle* h, const unsigned int* d_off, unsigned int* flag, size_t NC, size_t N, const char* scan_name, const char* offsets_name, const char* scatter_name) {
        if (!out_off) return LK_OK;
        c.off = d_off, c.flag = flag, c.n_clouds = (unsigned int)NC, c.total = (unsigned int)N;
        h_off.resize(NC + 1);
        size_t tb = h->prim_tmp.cap;
        hipError_t scanned = hipSuccess;
        LAUNCH(h, scan_name, scanned = lk_prim_exclusive_scan(h->prim_tmp.p, tb, c.flag, c.scan, N + 1, h->stream));
        HIPCHK(h, scanned);
        LAUNCH(h, offsets_name, hipLaunchKernelGGL(lk_c2c_compact_offsets_kernel, c2c_blocks(NC + 1), dim3(256), 0, h->stream, c));
        HIPCHK(h, hipMemcpyAsync(h_off.data(), c.out_off, 4 * (NC + 1), hipMemcpyDeviceToHost, h->stream));
        if (moved && N) LAUNCH(h, scatter_name, hipLaunchKernelGGL(lk_c2c_compact_scatter_kernel, c2c_blocks(N), dim3(256), 0, h->stream, c));
        return LK_OK;
    }
    // after the synchronisation.  *n_out: records written to out_cloud / src_idx
    void finish(size_t* n_out) const {
        for (size_t k = 0; k < h_off.size(); ++k) out_off[k] = h_off[k];
        if (n_out) *n_out = h_off.empty() ? 0 : h_off.back();
    }
};

// what both entries refuse before anything is launched
static int mme_check(lk_handle* h, const char* who, const MmeArgs& a, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    LKCHK(clouds_check_args(h, w, a.clouds, a.n_clouds, a.off, a.out, cloud_align));
    if ((uintptr_t)a.n & 3) return fail(h, LK_ERR_INVALID, w + "n must be 4-byte aligned");
    if ((uintptr_t)a.hh & 7) return fail(h, LK_ERR_INVALID, w + "h must be 8-byte aligned");
    if ((uintptr_t)a.lmin & 7) return fail(h, LK_ERR_INVALID, w + "lmin must be 8-byte aligned");
    LKCHK(radius_check(h, w, "radius", a.radius));
    if (a.min_pts < 4) return fail(h, LK_ERR_INVALID, w + "min_pts is " + std::to_string(a.min_pts) + ": at least 4 (below four points det is 0 by rank)");
    LKCHK(clouds_check_table(h, w, a.n_clouds, a.off, total));
    const C2cSpan in = {"clouds", (uintptr_t)a.clouds + 16u * (uintptr_t)a.off[0], 16u * *total};
    const C2cSpan o[3] = {{"n", (uintptr_t)a.n, 4 * *total}, {"h", (uintptr_t)a.hh, 8 * *total}, {"lmin", (uintptr_t)a.lmin, 8 * *total}};
    for (int i = 0; i < 3; ++i) LKCHK(c2c_overlap_check(h, w, o[i], &in, 1, "the input clouds", o + i + 1, 2 - i));
    return LK_OK;
}

// the call behind mme_check, on DEVICE clouds and DEVICE per-point arrays (null: the library's own)
static int mme_run(lk_handle* h, const MmeArgs& a, size_t N) {
    const size_t NC = a.n_clouds;
    const std::vector<unsigned int> used = nonempty_clouds(a.off, NC);
    C2cIndex x = {};
    LkMmeCall m = {};
    LKCHK(c2c_carve(h, [&](LkCarve& c) {
        x.take(c, NC, used.size(), N);
        m.n = c2c_or_own(c, a.n, N), m.h = c2c_or_own(c, a.hh, N), m.lmin = c2c_or_own(c, a.lmin, N);
        m.out = c.take<lk_mme>(NC);
    }));
    LKCHK(c2c_index(h, reinterpret_cast<const float4*>(a.clouds), a.off, NC, used, a.radius, x));
    m.off = x.d_off, m.status = x.status, m.grid = x.grid, m.keys = x.k1, m.recs = x.recs;
    m.reach2 = lk_c2c_reach2(a.radius);
    m.n_clouds = (unsigned int)NC, m.min_pts = a.min_pts, m.total = (unsigned int)N;
    if (N) LAUNCH(h, "mme_point", hipLaunchKernelGGL(lk_mme_point_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
    LAUNCH(h, "mme_reduce", hipLaunchKernelGGL(lk_mme_reduce_kernel, dim3((unsigned int)NC), dim3(256), 0, h->stream, m));
    std::vector<lk_mme> rec(NC);
    HIPCHK(h, hipMemcpyAsync(rec.data(), m.out, sizeof(lk_mme) * NC, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(a.out, rec.data(), sizeof(lk_mme) * NC);
    return LK_OK;
}

extern "C" {

int lk_clouds_mme_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts, lk_mme* out, uint32_t* d_n,
                      double* d_h, double* d_lmin) {
    CHECK_H(h);
    const MmeArgs a = {d_clouds, n_clouds, off, radius, min_pts, out, d_n, d_h, d_lmin};
    size_t total = 0;
    LKCHK(mme_check(h, "lk_clouds_mme_dev", a, 16, &total));
    return mme_run(h, a, total);
}

int lk_clouds_mme(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts, lk_mme* out, uint32_t* n, double* hh,
                  double* lmin) {
    CHECK_H(h);
    MmeArgs a = {clouds, n_clouds, off, radius, min_pts, out, n, hh, lmin};
    size_t total = 0;
    LKCHK(mme_check(h, "lk_clouds_mme", a, 4, &total));
    C2cStage st;
    st.out = {{n, 4, total}, {hh, 8, total}, {lmin, 8, total}};
    LKCHK(st.upload_clouds(h, a.clouds, a.n_clouds, a.off));
    a.n = st.out[0], a.hh = st.out[1], a.lmin = st.out[2];
    LKCHK(mme_run(h, a, total));
    return st.fetch(h);
}

}  // extern "C"

namespace {
struct NormalsArgs {   // the arguments both entries share, as the caller gave them
    const float* clouds;
    size_t n_clouds;
    const uint64_t* off;
    double radius;
    uint32_t min_pts;
    double min_planarity;
    lk_normals* out;
    float* normals;
};
}  // namespace

// what both entries refuse before anything is launched: the clouds' refusals with the radius where lk_clouds_mme(_dev) has it, then the entry's own
static int normals_check(lk_handle* h, const char* who, const NormalsArgs& a, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    LKCHK(clouds_check_args(h, w, a.clouds, a.n_clouds, a.off, a.out, cloud_align));
    LKCHK(radius_check(h, w, "radius", a.radius));
    LKCHK(clouds_check_table(h, w, a.n_clouds, a.off, total));
    if (a.min_pts < 3) return fail(h, LK_ERR_INVALID, w + "min_pts is " + std::to_string(a.min_pts) + ": at least 3 (two points span no plane)");
    if (!std::isfinite(a.min_planarity) || a.min_planarity < 0.0 || a.min_planarity > 1.0) return fail(h, LK_ERR_INVALID, w + "min_planarity must be finite and in 0 .. 1");
    if (!a.normals) return fail(h, LK_ERR_INVALID, w + "null argument (normals)");
    if ((uintptr_t)a.normals & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "normals must be " + std::to_string(cloud_align) + "-byte aligned");
    const C2cSpan in = {"clouds", (uintptr_t)a.clouds + 16u * (uintptr_t)a.off[0], 16u * *total}, o = {"normals", (uintptr_t)a.normals, 16u * *total};
    return c2c_overlap_check(h, w, o, &in, 1, "the input clouds", nullptr, 0);
}

// the call behind normals_check, on DEVICE clouds and a DEVICE record array
static int normals_run(lk_handle* h, const NormalsArgs& a, size_t N) {
    const size_t NC = a.n_clouds;
    const std::vector<unsigned int> used = nonempty_clouds(a.off, NC);
    C2cIndex x = {};
    LkNormalsCall m = {};
    LKCHK(c2c_carve(h, [&](LkCarve& c) { x.take(c, NC, used.size(), N), m.out = c.take<lk_normals>(NC); }));
    LKCHK(c2c_index(h, reinterpret_cast<const float4*>(a.clouds), a.off, NC, used, a.radius, x));
    m.off = x.d_off, m.status = x.status, m.grid = x.grid, m.keys = x.k1, m.recs = x.recs, m.normals = reinterpret_cast<float4*>(a.normals);
    m.reach2 = lk_c2c_reach2(a.radius), m.min_planarity = a.min_planarity;
    m.n_clouds = (unsigned int)NC, m.min_pts = a.min_pts, m.total = (unsigned int)N;
    if (N) LAUNCH(h, "normals_point", hipLaunchKernelGGL(lk_normals_point_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
    LAUNCH(h, "normals_count", hipLaunchKernelGGL(lk_normals_count_kernel, dim3((unsigned int)NC), dim3(256), 0, h->stream, m));
    std::vector<lk_normals> rec(NC);
    HIPCHK(h, hipMemcpyAsync(rec.data(), m.out, sizeof(lk_normals) * NC, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(a.out, rec.data(), sizeof(lk_normals) * NC);
    return LK_OK;
}

extern "C" {

int lk_clouds_normals_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts, double min_planarity,
                          lk_normals* out, float* d_normals) {
    CHECK_H(h);
    const NormalsArgs a = {d_clouds, n_clouds, off, radius, min_pts, min_planarity, out, d_normals};
    size_t total = 0;
    LKCHK(normals_check(h, "lk_clouds_normals_dev", a, 16, &total));
    return normals_run(h, a, total);
}

int lk_clouds_normals(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double radius, uint32_t min_pts, double min_planarity, lk_normals* out,
                      float* normals) {
    CHECK_H(h);
    NormalsArgs a = {clouds, n_clouds, off, radius, min_pts, min_planarity, out, normals};
    size_t total = 0;
    LKCHK(normals_check(h, "lk_clouds_normals", a, 4, &total));
    C2cStage st;
    st.out = {{normals, 16, total}};
    LKCHK(st.upload_clouds(h, a.clouds, a.n_clouds, a.off));
    a.normals = st.out[0];
    LKCHK(normals_run(h, a, total));
    return st.fetch(h);
}

}  // extern "C"

namespace {
struct SorArgs {   // the arguments both entries share, as the caller gave them
    const float* clouds;
    size_t n_clouds;
    const uint64_t* off;
    uint32_t k;
    double reach, n_sigma;
    lk_sor* out;
    float* out_cloud;
    uint64_t* out_off;
    uint32_t* src_idx;
    uint8_t* keep;
    uint32_t* cnt;
    double* dbar;
};
}  // namespace

// what both entries refuse before anything is launched: the reach, the clouds' refusals, then the entry's own
static int sor_check(lk_handle* h, const char* who, const SorArgs& a, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    LKCHK(radius_check(h, w, "reach", a.reach));
    LKCHK(clouds_check_args(h, w, a.clouds, a.n_clouds, a.off, a.out, cloud_align));
    LKCHK(clouds_check_table(h, w, a.n_clouds, a.off, total));
    if (a.k == 0 || a.k > LK_SOR_MAX_K) return fail(h, LK_ERR_INVALID, w + "k is " + std::to_string(a.k) + ": 1 .. " + std::to_string(LK_SOR_MAX_K));
    if (!(a.n_sigma >= 0.0)) return fail(h, LK_ERR_INVALID, w + "n_sigma must be 0 or above (+inf: the radius criterion alone)");
    if (a.out_cloud && !a.out_off) return fail(h, LK_ERR_INVALID, w + "out_cloud needs out_off");
    if (a.src_idx && !a.out_off) return fail(h, LK_ERR_INVALID, w + "src_idx needs out_off");
    if ((uintptr_t)a.out_cloud & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "out_cloud must be " + std::to_string(cloud_align) + "-byte aligned");
    if ((uintptr_t)a.src_idx & 3) return fail(h, LK_ERR_INVALID, w + "src_idx must be 4-byte aligned");
    if ((uintptr_t)a.cnt & 3) return fail(h, LK_ERR_INVALID, w + "cnt must be 4-byte aligned");
    if ((uintptr_t)a.dbar & 7) return fail(h, LK_ERR_INVALID, w + "dbar must be 8-byte aligned");
    const C2cSpan in = {"clouds", (uintptr_t)a.clouds + 16u * (uintptr_t)a.off[0], 16u * *total};
    const C2cSpan o[5] = {{"out_cloud", (uintptr_t)a.out_cloud, 16 * *total}, {"src_idx", (uintptr_t)a.src_idx, 4 * *total}, {"keep", (uintptr_t)a.keep, *total},
                          {"cnt", (uintptr_t)a.cnt, 4 * *total}, {"dbar", (uintptr_t)a.dbar, 8 * *total}};
    for (int i = 0; i < 5; ++i) LKCHK(c2c_overlap_check(h, w, o[i], &in, 1, "the input clouds", o + i + 1, 4 - i));
    return LK_OK;
}

template <int CAP>
static void sor_point_launch(lk_handle* h, const LkSorCall& m, size_t N) {
    hipLaunchKernelGGL(lk_sor_point_kernel<CAP>, c2c_blocks(N), dim3(256), 0, h->stream, m);
}

// the call behind sor_check, on DEVICE clouds and DEVICE outputs (null: not asked for; what a later kernel needs is then the library's own).
// *n_out: records written to out_cloud / src_idx
static int sor_run(lk_handle* h, const SorArgs& a, size_t N, size_t* n_out) {
    const size_t NC = a.n_clouds;
    const std::vector<unsigned int> used = nonempty_clouds(a.off, NC);
    const bool flags = a.keep || a.out_off;
    C2cIndex x = {};
    LkSorCall m = {};
    C2cTail t(a.clouds, a.off, a.out_cloud, a.out_off, a.src_idx);
    LKCHK(c2c_carve(h, [&](LkCarve& c) {
        x.take(c, NC, used.size(), N);
        m.dbar = c2c_or_own(c, a.dbar, N);
        m.flag = c.take<unsigned int>(flags ? N + 1 : 0), m.thr = c.take<double>(NC), m.out = c.take<lk_sor>(NC);
        t.take(c, NC, N);
    }));
    if (a.out_off) LKCHK(scan_reserve(h, m.flag, t.c.scan, N + 1));
    LKCHK(c2c_index(h, reinterpret_cast<const float4*>(a.clouds), a.off, NC, used, a.reach, x));
    m.off = x.d_off, m.status = x.status, m.grid = x.grid, m.keys = x.k1, m.recs = x.recs;
    m.cnt = a.cnt, m.keep = a.keep;
    m.reach2 = lk_c2c_reach2(a.reach), m.n_sigma = a.n_sigma;
    m.n_clouds = (unsigned int)NC, m.k = a.k, m.total = (unsigned int)N;
    if (N) {
        const int cap = lk_sor_cap_of(a.k);
        if (cap == LK_SOR_CAP_SMALL) LAUNCH(h, "sor_point", sor_point_launch<LK_SOR_CAP_SMALL>(h, m, N));
        else if (cap == LK_SOR_CAP_MID) LAUNCH(h, "sor_point", sor_point_launch<LK_SOR_CAP_MID>(h, m, N));
        else LAUNCH(h, "sor_point", sor_point_launch<LK_SOR_CAP_BIG>(h, m, N));
    }
    LAUNCH(h, "sor_stats", hipLaunchKernelGGL(lk_sor_stats_kernel, dim3((unsigned int)NC), dim3(256), 0, h->stream, m));
    std::vector<lk_sor> rec(NC);
    HIPCHK(h, hipMemcpyAsync(rec.data(), m.out, sizeof(lk_sor) * NC, hipMemcpyDeviceToHost, h->stream));
    if (flags) LAUNCH(h, "sor_flag", hipLaunchKernelGGL(lk_sor_flag_kernel, c2c_blocks(N + 1), dim3(256), 0, h->stream, m));
    LKCHK(t.enqueue(h, m.off, m.flag, NC, N, "sor_scan", "sor_offsets", "sor_scatter"));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(a.out, rec.data(), sizeof(lk_sor) * NC);
    t.finish(n_out);
    return LK_OK;
}

extern "C" {

int lk_clouds_sor_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, uint32_t k, double reach, double n_sigma, lk_sor* out, float* d_out,
                      uint64_t* out_off, uint32_t* d_src_idx, uint8_t* d_keep, uint32_t* d_cnt, double* d_dbar) {
    CHECK_H(h);
    const SorArgs a = {d_clouds, n_clouds, off, k, reach, n_sigma, out, d_out, out_off, d_src_idx, d_keep, d_cnt, d_dbar};
    size_t total = 0;
    LKCHK(sor_check(h, "lk_clouds_sor_dev", a, 16, &total));
    return sor_run(h, a, total, nullptr);
}

int lk_clouds_sor(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, uint32_t k, double reach, double n_sigma, lk_sor* out, float* out_cloud,
                  uint64_t* out_off, uint32_t* src_idx, uint8_t* keep, uint32_t* cnt, double* dbar) {
    CHECK_H(h);
    SorArgs a = {clouds, n_clouds, off, k, reach, n_sigma, out, out_cloud, out_off, src_idx, keep, cnt, dbar};
    size_t total = 0, n_out = 0;
    LKCHK(sor_check(h, "lk_clouds_sor", a, 4, &total));
    C2cStage st;
    st.out = {{out_cloud, 16, total}, {src_idx, 4, total}, {keep, 1, total}, {cnt, 4, total}, {dbar, 8, total}};
    LKCHK(st.upload_clouds(h, a.clouds, a.n_clouds, a.off));
    a.out_cloud = st.out[0], a.src_idx = st.out[1], a.keep = st.out[2], a.cnt = st.out[3], a.dbar = st.out[4];
    LKCHK(sor_run(h, a, total, &n_out));
    st.out[0].count = st.out[1].count = n_out;   // nothing behind the kept records is written
    return st.fetch(h);
}

}  // extern "C"

namespace {
struct ClusterArgs {   // the arguments both entries share, as the caller gave them
    const float* clouds;
    size_t n_clouds;
    const uint64_t* off;
    double reach;
    uint32_t min_pts, min_size, max_size, flags;
    lk_cluster* out;
    uint32_t* label;
    uint8_t* kind;
    uint32_t *n, *cl_size, *cl_first;
    uint64_t* cl_off;
    float* out_cloud;
    uint64_t* out_off;
    uint32_t* src_idx;
};
}  // namespace

// what both entries refuse before anything is launched: the reach, the clouds' refusals, then the entry's own
static int cluster_check(lk_handle* h, const char* who, const ClusterArgs& a, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    LKCHK(radius_check(h, w, "reach", a.reach));
    LKCHK(clouds_check_args(h, w, a.clouds, a.n_clouds, a.off, a.out, cloud_align));
    LKCHK(clouds_check_table(h, w, a.n_clouds, a.off, total));
    if (a.min_pts == 0) return fail(h, LK_ERR_INVALID, w + "min_pts is 0: at least 1 (a point counts itself)");
    if (a.min_size > a.max_size) return fail(h, LK_ERR_INVALID, w + "min_size is " + std::to_string(a.min_size) + ", above max_size " + std::to_string(a.max_size));
    if (a.flags & ~LK_CLUSTER_KEEP_LARGEST) return fail(h, LK_ERR_INVALID, w + "flags holds an unknown bit: 0 or LK_CLUSTER_KEEP_LARGEST");
    if (a.cl_size && !a.cl_off) return fail(h, LK_ERR_INVALID, w + "cl_size needs cl_off");
    if (a.cl_first && !a.cl_off) return fail(h, LK_ERR_INVALID, w + "cl_first needs cl_off");
    if (a.out_cloud && !a.out_off) return fail(h, LK_ERR_INVALID, w + "out_cloud needs out_off");
    if (a.src_idx && !a.out_off) return fail(h, LK_ERR_INVALID, w + "src_idx needs out_off");
    if ((uintptr_t)a.out_cloud & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "out_cloud must be " + std::to_string(cloud_align) + "-byte aligned");
    const C2cSpan in = {"clouds", (uintptr_t)a.clouds + 16u * (uintptr_t)a.off[0], 16u * *total};
    const C2cSpan o[7] = {{"out_cloud", (uintptr_t)a.out_cloud, 16 * *total}, {"src_idx", (uintptr_t)a.src_idx, 4 * *total}, {"label", (uintptr_t)a.label, 4 * *total},
                          {"kind", (uintptr_t)a.kind, *total}, {"n", (uintptr_t)a.n, 4 * *total}, {"cl_size", (uintptr_t)a.cl_size, 4 * *total},
                          {"cl_first", (uintptr_t)a.cl_first, 4 * *total}};
    for (int i = 1; i < 7; ++i)
        if (i != 3 && (o[i].p & 3)) return fail(h, LK_ERR_INVALID, w + o[i].name + " must be 4-byte aligned");
    for (int i = 0; i < 7; ++i) LKCHK(c2c_overlap_check(h, w, o[i], &in, 1, "the input clouds", o + i + 1, 6 - i));
    return LK_OK;
}

// the call behind cluster_check, on DEVICE clouds and DEVICE outputs (null: not asked for; what a later kernel needs is then the library's own).
// *n_cl: entries written to cl_size / cl_first, *n_out: records written to out_cloud / src_idx
static int cluster_run(lk_handle* h, const ClusterArgs& a, size_t N, size_t* n_cl, size_t* n_out) {
    const size_t NC = a.n_clouds;
    const std::vector<unsigned int> used = nonempty_clouds(a.off, NC);
    C2cIndex x = {};
    LkClusterCall m = {};
    C2cTail t(a.clouds, a.off, a.out_cloud, a.out_off, a.src_idx);
    LKCHK(c2c_carve(h, [&](LkCarve& c) {
        x.take(c, NC, used.size(), N);
        m.core = c.take<unsigned char>(N), m.parent = c.take<unsigned int>(N), m.root = c.take<unsigned int>(N);
        m.n = c2c_or_own(c, a.n, N), m.kind = c2c_or_own(c, a.kind, N);
        m.rflag = c.take<unsigned int>(N + 1), m.rscan = c.take<unsigned int>(N + 1), m.size = c.take<unsigned int>(N), m.first = c.take<unsigned int>(N);
        m.cl_off = c.take<unsigned int>(NC + 1), m.kept_id = c.take<unsigned int>(NC);
        m.flag = c.take<unsigned int>(a.out_off ? N + 1 : 0), m.out = c.take<lk_cluster>(NC);
        t.take(c, NC, N);
    }));
    LKCHK(scan_reserve(h, m.rflag, m.rscan, N + 1));   // (the tail's scan is as long)
    LKCHK(c2c_index(h, reinterpret_cast<const float4*>(a.clouds), a.off, NC, used, a.reach, x));
    m.off = x.d_off, m.status = x.status, m.grid = x.grid, m.keys = x.k1, m.recs = x.recs;
    m.label = a.label, m.cl_size = a.cl_size, m.cl_first = a.cl_first;
    m.reach2 = lk_c2c_reach2(a.reach);
    m.n_clouds = (unsigned int)NC, m.total = (unsigned int)N, m.min_pts = a.min_pts, m.min_size = a.min_size, m.max_size = a.max_size;
    m.keep_largest = a.flags & LK_CLUSTER_KEEP_LARGEST;
    if (N) {
        LAUNCH(h, "cluster_count", hipLaunchKernelGGL(lk_cluster_count_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
        LAUNCH(h, "cluster_link", hipLaunchKernelGGL(lk_cluster_link_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
        LAUNCH(h, "cluster_assign", hipLaunchKernelGGL(lk_cluster_assign_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
        HIPCHK(h, hipMemsetAsync(m.size, 0, 4 * N, h->stream));
    }
    LAUNCH(h, "cluster_rootflag", hipLaunchKernelGGL(lk_cluster_rootflag_kernel, c2c_blocks(N + 1), dim3(256), 0, h->stream, m));
    size_t tb = h->prim_tmp.cap;
    hipError_t scanned = hipSuccess;
    LAUNCH(h, "cluster_ids", scanned = lk_prim_exclusive_scan(h->prim_tmp.p, tb, m.rflag, m.rscan, N + 1, h->stream));
    HIPCHK(h, scanned);
    if (N) LAUNCH(h, "cluster_label", hipLaunchKernelGGL(lk_cluster_label_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
    LAUNCH(h, "cluster_record", hipLaunchKernelGGL(lk_cluster_record_kernel, dim3((unsigned int)NC), dim3(256), 0, h->stream, m));
    LAUNCH(h, "cluster_tables", hipLaunchKernelGGL(lk_cluster_tables_kernel, c2c_blocks(std::max(N, NC + 1)), dim3(256), 0, h->stream, m));
    std::vector<lk_cluster> rec(NC);
    std::vector<unsigned int> coff(NC + 1);
    HIPCHK(h, hipMemcpyAsync(rec.data(), m.out, sizeof(lk_cluster) * NC, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(coff.data(), m.cl_off, 4 * (NC + 1), hipMemcpyDeviceToHost, h->stream));
    if (a.out_off) LAUNCH(h, "cluster_flag", hipLaunchKernelGGL(lk_cluster_flag_kernel, c2c_blocks(N + 1), dim3(256), 0, h->stream, m));
    LKCHK(t.enqueue(h, m.off, m.flag, NC, N, "cluster_scan", "cluster_offsets", "cluster_scatter"));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(a.out, rec.data(), sizeof(lk_cluster) * NC);
    if (a.cl_off)
        for (size_t c = 0; c <= NC; ++c) a.cl_off[c] = coff[c];
    if (n_cl) *n_cl = coff[NC];
    t.finish(n_out);
    return LK_OK;
}

extern "C" {

int lk_clouds_cluster_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double reach, uint32_t min_pts, uint32_t min_size,
                          uint32_t max_size, uint32_t flags, lk_cluster* out, uint32_t* d_label, uint8_t* d_kind, uint32_t* d_n, uint32_t* d_cl_size,
                          uint32_t* d_cl_first, uint64_t* cl_off, float* d_out, uint64_t* out_off, uint32_t* d_src_idx) {
    CHECK_H(h);
    const ClusterArgs a = {d_clouds, n_clouds, off, reach, min_pts, min_size, max_size, flags, out, d_label, d_kind, d_n, d_cl_size, d_cl_first, cl_off, d_out, out_off, d_src_idx};
    size_t total = 0;
    LKCHK(cluster_check(h, "lk_clouds_cluster_dev", a, 16, &total));
    return cluster_run(h, a, total, nullptr, nullptr);
}

int lk_clouds_cluster(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double reach, uint32_t min_pts, uint32_t min_size,
                      uint32_t max_size, uint32_t flags, lk_cluster* out, uint32_t* label, uint8_t* kind, uint32_t* n, uint32_t* cl_size, uint32_t* cl_first,
                      uint64_t* cl_off, float* out_cloud, uint64_t* out_off, uint32_t* src_idx) {
    CHECK_H(h);
    ClusterArgs a = {clouds, n_clouds, off, reach, min_pts, min_size, max_size, flags, out, label, kind, n, cl_size, cl_first, cl_off, out_cloud, out_off, src_idx};
    size_t total = 0, n_cl = 0, n_out = 0;
    LKCHK(cluster_check(h, "lk_clouds_cluster", a, 4, &total));
    C2cStage st;
    st.out = {{label, 4, total}, {kind, 1, total}, {n, 4, total}, {cl_size, 4, total}, {cl_first, 4, total}, {out_cloud, 16, total}, {src_idx, 4, total}};
    LKCHK(st.upload_clouds(h, a.clouds, a.n_clouds, a.off));
    a.label = st.out[0], a.kind = st.out[1], a.n = st.out[2], a.cl_size = st.out[3], a.cl_first = st.out[4], a.out_cloud = st.out[5], a.src_idx = st.out[6];
    LKCHK(cluster_run(h, a, total, &n_cl, &n_out));
    st.out[3].count = st.out[4].count = n_cl, st.out[5].count = st.out[6].count = n_out;   // nothing behind the clusters and the kept records is written
    return st.fetch(h);
}

}  // extern "C"

namespace {
struct PlanesArgs {   // the arguments both entries share, as the caller gave them
    const float* clouds;
    size_t n_clouds;
    const uint64_t* off;
    double dist;
    uint32_t n_hyp, max_planes, min_inliers;
    const double* axis;
    double cos_max_angle;
    uint64_t seed;
    uint32_t flags;
    lk_planes* out;
    lk_plane* planes;
    uint32_t* label;
    float* out_cloud;
    uint64_t* out_off;
    uint32_t* src_idx;
};
}  // namespace

// what both entries refuse before anything is launched: the clouds' refusals, then the entry's own
static int planes_check(lk_handle* h, const char* who, const PlanesArgs& a, unsigned int cloud_align, size_t* total) {
    const std::string w = std::string(who) + ": ";
    LKCHK(clouds_check_args(h, w, a.clouds, a.n_clouds, a.off, a.out, cloud_align));
    LKCHK(clouds_check_table(h, w, a.n_clouds, a.off, total));
    if (!a.planes) return fail(h, LK_ERR_INVALID, w + "null argument (planes)");
    if (!std::isfinite(a.dist) || !(a.dist > 0.0)) return fail(h, LK_ERR_INVALID, w + "dist must be finite and above 0");
    if (a.n_hyp == 0 || a.n_hyp > LK_PLANES_MAX_HYP) return fail(h, LK_ERR_INVALID, w + "n_hyp is " + std::to_string(a.n_hyp) + ": 1 .. LK_PLANES_MAX_HYP");
    if (a.max_planes == 0 || a.max_planes > LK_PLANES_MAX_PLANES)
        return fail(h, LK_ERR_INVALID, w + "max_planes is " + std::to_string(a.max_planes) + ": 1 .. LK_PLANES_MAX_PLANES");
    if (a.min_inliers < 3) return fail(h, LK_ERR_INVALID, w + "min_inliers is " + std::to_string(a.min_inliers) + ": at least 3 (the sample points count)");
    if (a.axis) {
        const bool finite = std::isfinite(a.axis[0]) && std::isfinite(a.axis[1]) && std::isfinite(a.axis[2]);
        const double aa = finite ? lk_planes_axis(a.axis, 0.0).aa : 0.0;
        if (!finite || !(aa > 0.0) || !std::isfinite(aa)) return fail(h, LK_ERR_INVALID, w + "axis must be finite and not zero");
    }
    if (!(a.cos_max_angle >= 0.0 && a.cos_max_angle <= 1.0)) return fail(h, LK_ERR_INVALID, w + "cos_max_angle must lie in 0 .. 1");
    if (a.flags & ~LK_PLANES_KEEP_PLANES) return fail(h, LK_ERR_INVALID, w + "flags holds an unknown bit: 0 or LK_PLANES_KEEP_PLANES");
    if (a.out_cloud && !a.out_off) return fail(h, LK_ERR_INVALID, w + "out_cloud needs out_off");
    if (a.src_idx && !a.out_off) return fail(h, LK_ERR_INVALID, w + "src_idx needs out_off");
    if ((uintptr_t)a.out_cloud & (cloud_align - 1)) return fail(h, LK_ERR_INVALID, w + "out_cloud must be " + std::to_string(cloud_align) + "-byte aligned");
    const C2cSpan in = {"clouds", (uintptr_t)a.clouds + 16u * (uintptr_t)a.off[0], 16u * *total};
    const C2cSpan o[3] = {{"out_cloud", (uintptr_t)a.out_cloud, 16 * *total}, {"src_idx", (uintptr_t)a.src_idx, 4 * *total}, {"label", (uintptr_t)a.label, 4 * *total}};
    for (int i = 1; i < 3; ++i)
        if (o[i].p & 3) return fail(h, LK_ERR_INVALID, w + o[i].name + " must be 4-byte aligned");
    for (int i = 0; i < 3; ++i) LKCHK(c2c_overlap_check(h, w, o[i], &in, 1, "the input clouds", o + i + 1, 2 - i));
    return LK_OK;
}

// the call behind planes_check, on DEVICE clouds and DEVICE outputs (null: not asked for).  *n_out: records written to out_cloud / src_idx
static int planes_run(lk_handle* h, const PlanesArgs& a, size_t N, size_t* n_out) {
    const size_t NC = a.n_clouds, NP = NC * a.max_planes;
    const std::vector<unsigned int> used = nonempty_clouds(a.off, NC);
    std::vector<unsigned int> roff(NC + 1), cfirst(NC + 1, 0u);   // the table from the first record; the score blocks in front of a cloud
    for (size_t c = 0; c < NC; ++c) cfirst[c + 1] = cfirst[c] + (unsigned int)((a.off[c + 1] - a.off[c] + LK_PLANES_CHUNK - 1) / LK_PLANES_CHUNK);
    for (size_t c = 0; c <= NC; ++c) roff[c] = (unsigned int)(a.off[c] - a.off[0]);
    unsigned long long* d_off64 = nullptr;
    unsigned int *d_off = nullptr, *d_used = nullptr, *d_status = nullptr, *d_cfirst = nullptr;
    int* d_mm = nullptr;
    LkPlanesCall m = {};
    C2cTail t(a.clouds, a.off, a.out_cloud, a.out_off, a.src_idx);
    LKCHK(c2c_carve(h, [&](LkCarve& c) {
        d_off64 = c.take<unsigned long long>(NC + 1), d_off = c.take<unsigned int>(NC + 1), d_used = c.take<unsigned int>(used.size());
        d_cfirst = c.take<unsigned int>(NC + 1), d_status = c.take<unsigned int>(NC), d_mm = c.take<int>(6 * NC);
        m.flag = c.take<unsigned int>(N + 1), m.scan = c.take<unsigned int>(N + 1), m.rem = c.take<float4>(N), m.label = c2c_or_own(c, a.label, N);
        m.score = c.take<unsigned int>(NC * a.n_hyp), m.done = c.take<unsigned int>(NC), m.n_planes = c.take<unsigned int>(NC), m.win_h = c.take<unsigned int>(NC);
        m.win = c.take<LkPlanesHyp>(NC), m.planes = c.take<lk_plane>(NP), m.csum = c.take<double>(6 * NP), m.out = c.take<lk_planes>(NC);
        t.take(c, NC, N, false), t.c.scan = m.scan;   // the rounds' scan array: free again when the tail runs
    }));
    LKCHK(scan_reserve(h, m.flag, m.scan, N + 1));
    HIPCHK(h, hipMemcpyAsync(d_off64, a.off, 8 * (NC + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_off, roff.data(), 4 * (NC + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_cfirst, cfirst.data(), 4 * (NC + 1), hipMemcpyHostToDevice, h->stream));
    if (!used.empty()) HIPCHK(h, hipMemcpyAsync(d_used, used.data(), 4 * used.size(), hipMemcpyHostToDevice, h->stream));
    // the status words: lk_c2c_out_of_range at an edge of 1 is |coordinate| >= 2^30
    LKCHK(c2c_bounds(h, reinterpret_cast<const float4*>(a.clouds), a.off, NC, used, d_off64, d_used, 1.0, d_mm, d_status));
    m.off = d_off, m.status = d_status, m.chunk_first = d_cfirst, m.in = reinterpret_cast<const float4*>(a.clouds) + a.off[0];
    m.axis = lk_planes_axis(a.axis, a.cos_max_angle), m.dist2 = a.dist * a.dist, m.seed = a.seed;
    m.n_clouds = (unsigned int)NC, m.total = (unsigned int)N, m.n_hyp = a.n_hyp, m.max_planes = a.max_planes, m.min_inliers = a.min_inliers;
    m.keep_planes = a.flags & LK_PLANES_KEEP_PLANES;
    HIPCHK(h, hipMemsetAsync(m.done, 0, 4 * NC, h->stream));
    HIPCHK(h, hipMemsetAsync(m.n_planes, 0, 4 * NC, h->stream));
    HIPCHK(h, hipMemsetAsync(m.planes, 0, sizeof(lk_plane) * NP, h->stream));
    LAUNCH(h, "planes_init", hipLaunchKernelGGL(lk_planes_init_kernel, c2c_blocks(N + 1), dim3(256), 0, h->stream, m));
    const dim3 score_grid(cfirst[NC], (a.n_hyp + LK_PLANES_GROUP - 1) / LK_PLANES_GROUP);
    size_t tb = 0;
    hipError_t scanned = hipSuccess;
    for (uint32_t r = 0; r < a.max_planes && N; ++r) {
        m.round = r;
        tb = h->prim_tmp.cap;
        LAUNCH(h, "planes_scan", scanned = lk_prim_exclusive_scan(h->prim_tmp.p, tb, m.flag, m.scan, N + 1, h->stream));
        HIPCHK(h, scanned);
        LAUNCH(h, "planes_compact", hipLaunchKernelGGL(lk_planes_compact_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
        HIPCHK(h, hipMemsetAsync(m.score, 0, 4 * NC * a.n_hyp, h->stream));
        LAUNCH(h, "planes_score", hipLaunchKernelGGL(lk_planes_score_kernel, score_grid, dim3(256), 0, h->stream, m));
        LAUNCH(h, "planes_argmax", hipLaunchKernelGGL(lk_planes_argmax_kernel, dim3((unsigned int)NC), dim3(64), 0, h->stream, m));
        LAUNCH(h, "planes_mark", hipLaunchKernelGGL(lk_planes_mark_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
    }
    if (N) {
        LAUNCH(h, "planes_refit", hipLaunchKernelGGL(lk_planes_refit_kernel, dim3((unsigned int)NC, a.max_planes), dim3(256), 0, h->stream, m));
        LAUNCH(h, "planes_fit", hipLaunchKernelGGL(lk_planes_fit_kernel, c2c_blocks(NP), dim3(256), 0, h->stream, m));
    }
    LAUNCH(h, "planes_record", hipLaunchKernelGGL(lk_planes_record_kernel, c2c_blocks(NC), dim3(256), 0, h->stream, m));
    std::vector<lk_planes> rec(NC);
    std::vector<lk_plane> prec(NP);
    HIPCHK(h, hipMemcpyAsync(rec.data(), m.out, sizeof(lk_planes) * NC, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(prec.data(), m.planes, sizeof(lk_plane) * NP, hipMemcpyDeviceToHost, h->stream));
    if (a.out_off && N) LAUNCH(h, "planes_keep", hipLaunchKernelGGL(lk_planes_keep_kernel, c2c_blocks(N), dim3(256), 0, h->stream, m));
    LKCHK(t.enqueue(h, m.off, m.flag, NC, N, "planes_keep_scan", "planes_offsets", "planes_scatter"));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(a.out, rec.data(), sizeof(lk_planes) * NC);
    memcpy(a.planes, prec.data(), sizeof(lk_plane) * NP);
    t.finish(n_out);
    return LK_OK;
}

extern "C" {

int lk_clouds_planes_dev(lk_handle* h, const float* d_clouds, size_t n_clouds, const uint64_t* off, double dist, uint32_t n_hyp, uint32_t max_planes,
                         uint32_t min_inliers, const double* axis, double cos_max_angle, uint64_t seed, uint32_t flags, lk_planes* out, lk_plane* planes,
                         uint32_t* d_label, float* d_out, uint64_t* out_off, uint32_t* d_src_idx) {
    CHECK_H(h);
    const PlanesArgs a = {d_clouds, n_clouds, off, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, out, planes, d_label, d_out, out_off, d_src_idx};
    size_t total = 0;
    LKCHK(planes_check(h, "lk_clouds_planes_dev", a, 16, &total));
    return planes_run(h, a, total, nullptr);
}

int lk_clouds_planes(lk_handle* h, const float* clouds, size_t n_clouds, const uint64_t* off, double dist, uint32_t n_hyp, uint32_t max_planes,
                     uint32_t min_inliers, const double* axis, double cos_max_angle, uint64_t seed, uint32_t flags, lk_planes* out, lk_plane* planes,
                     uint32_t* label, float* out_cloud, uint64_t* out_off, uint32_t* src_idx) {
    CHECK_H(h);
    PlanesArgs a = {clouds, n_clouds, off, dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, out, planes, label, out_cloud, out_off, src_idx};
    size_t total = 0, n_out = 0;
    LKCHK(planes_check(h, "lk_clouds_planes", a, 4, &total));
    C2cStage st;
    st.out = {{label, 4, total}, {out_cloud, 16, total}, {src_idx, 4, total}};
    LKCHK(st.upload_clouds(h, a.clouds, a.n_clouds, a.off));
    a.label = st.out[0], a.out_cloud = st.out[1], a.src_idx = st.out[2];
    LKCHK(planes_run(h, a, total, &n_out));
    st.out[1].count = st.out[2].count = n_out;   // nothing behind the kept records is written
    return st.fetch(h);
}

}  // extern "C"
