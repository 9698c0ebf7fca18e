// lk_pre_kernels.h — the two steps that feed the path, kept on the device so that a raw scan
// never returns to the host between decode and the ESKF update:
//   pcl::VoxelGrid centroid filter as used at KILO.cc:356-360  -> cell index, stable radix sort by cell, one thread
//       per cell sums its points sequentially in input order in float32 (all four fields incl. curvature)
//   std::sort by curvature at KILO.cc:369-370                   -> stable radix sort on the order-preserving bit image
// Definition (PCL leaves the order inside a cell and the output order undefined): oracle/preprocess_oracle.py.
// HBM-bound streaming kernels: one lk_point (16 B, float4) per lane, coalesced.
// ONE set of kernels for a scan and for a run of scans (front_decode / front_grid in legkilo_hip.hip): the kernels that must know a point's
// scan (lk_dscan_*, further down) take the run's tables, or null pointers when the call holds one message; lk_pre_starts / centroid / gather
// run over all cells of a call, whatever scans they belong to.
#pragma once
#include "lk_device.h"

__device__ __forceinline__ int lk_f2ord(float f) {
    int i = __float_as_int(f);
    return i >= 0 ? i : (i ^ 0x7fffffff);
}
__device__ __forceinline__ float lk_ord2f(int i) { return __int_as_float(i >= 0 ? i : (i ^ 0x7fffffff)); }

// mm[0..2] = min x,y,z ; mm[3..5] = max x,y,z   (order-preserving int image; init: INT_MAX / INT_MIN)
// a 256-thread block's per-lane bounds -> one atomicMin / atomicMax per field into mm (order-free: the result does not depend on the schedule)
__device__ __forceinline__ void lk_pre_minmax_merge(int lo[3], int hi[3], int* mm) {
    __shared__ int smin[3][4], smax[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[c] = min(lo[c], __shfl_xor(lo[c], o, LK_WAVE));
            hi[c] = max(hi[c], __shfl_xor(hi[c], o, LK_WAVE));
        }
        if ((threadIdx.x & 63) == 0) smin[c][threadIdx.x >> 6] = lo[c], smax[c][threadIdx.x >> 6] = hi[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        atomicMin(&mm[c], min(min(smin[c][0], smin[c][1]), min(smin[c][2], smin[c][3])));
        atomicMax(&mm[3 + c], max(max(smax[c][0], smax[c][1]), max(smax[c][2], smax[c][3])));
    }
}

// cell index idx = ijk0 + ijk1*div0 + ijk2*div0*div1 with ijk = floor(p * inv) - min_b (float arithmetic)
__device__ __forceinline__ void lk_cell_grid(const int* __restrict__ mm, float inv, int mn[3], int dv[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mn[c] = (int)floorf(lk_ord2f(mm[c]) * inv);
        dv[c] = (int)floorf(lk_ord2f(mm[3 + c]) * inv) - mn[c] + 1;
    }
}
__device__ __forceinline__ bool lk_cell_overflow(const int dv[3]) { return (double)dv[0] * (double)dv[1] * (double)dv[2] > 2147483647.0; }
__device__ __forceinline__ unsigned int lk_cell_key(float4 p, float inv, const int mn[3], const int dv[3]) {
    const int i0 = (int)floorf(p.x * inv) - mn[0], i1 = (int)floorf(p.y * inv) - mn[1], i2 = (int)floorf(p.z * inv) - mn[2];
    return (unsigned int)(i0 + i1 * dv[0] + i2 * dv[0] * dv[1]);
}

__global__ void __launch_bounds__(256)
    lk_pre_starts_kernel(const unsigned int* __restrict__ flags, const unsigned int* __restrict__ pos, int n, int* __restrict__ starts,
                         unsigned int* __restrict__ ncells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) starts[pos[i]] = i;
    if (i == n - 1) *ncells = pos[i] + flags[i];
}

// one thread per cell: sequential float32 sums in input order (vals are stably sorted by cell), centroid, time key
__global__ void __launch_bounds__(256)
    lk_pre_centroid_kernel(const lk_point* __restrict__ pts, const int* __restrict__ vals, const int* __restrict__ starts,
                           const unsigned int* __restrict__ ncells_p, int n, lk_point* __restrict__ cells,
                           unsigned int* __restrict__ tkeys, int* __restrict__ tvals) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int ncells = (int)*ncells_p;
    if (c >= ncells) return;
    const int b = starts[c], e = (c + 1 < ncells) ? starts[c + 1] : n;
    float sx = 0.f, sy = 0.f, sz = 0.f, sc = 0.f;
    for (int k = b; k < e; ++k) {
        const float4 p = reinterpret_cast<const float4*>(pts)[vals[k]];
        sx = sx + p.x, sy = sy + p.y, sz = sz + p.z, sc = sc + p.w;
    }
    const float cnt = (float)(e - b);
    const float4 o = make_float4(sx / cnt, sy / cnt, sz / cnt, sc / cnt);
    reinterpret_cast<float4*>(cells)[c] = o;
    unsigned int u = __float_as_uint(o.w);
    if (u == 0x80000000u) u = 0u;  // -0.0 (a sum of negative denormals that underflows in the division) and +0.0 are ONE time: a tie, kept in cell order
    tkeys[c] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving image of the float time stamp
    tvals[c] = c;
}

__global__ void __launch_bounds__(256)
    lk_pre_gather_kernel(const lk_point* __restrict__ cells, const int* __restrict__ order, int n, lk_point* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(cells)[order[i]];
}

// ------------------------------------------------------------------ sensor decode (lidar_processing.cc:25-108)
struct LkDecodeArgs {
    lk_cloud_layout lay;
    double time_scale;
    int filter_num;
    float blind;
};
__device__ __forceinline__ float lk_ld_f32(const unsigned char* p) {  // PointCloud2 fields are not 4-B aligned in general
    unsigned int u = (unsigned int)p[0] | ((unsigned int)p[1] << 8) | ((unsigned int)p[2] << 16) | ((unsigned int)p[3] << 24);
    return __uint_as_float(u);
}
__device__ __forceinline__ unsigned int lk_ld_u32(const unsigned char* p) {
    return (unsigned int)p[0] | ((unsigned int)p[1] << 8) | ((unsigned int)p[2] << 16) | ((unsigned int)p[3] << 24);
}
__device__ __forceinline__ double lk_ld_f64(const unsigned char* p) {
    unsigned long long u = (unsigned long long)lk_ld_u32(p) | ((unsigned long long)lk_ld_u32(p + 4) << 32);
    return __longlong_as_double((long long)u);
}
// keep flag of point i (counted from its message's first point) at p: every filter_num-th point outside the blind radius
__device__ __forceinline__ unsigned int lk_decode_keep(const unsigned char* p, int i, const LkDecodeArgs& a) {
    const float x = lk_ld_f32(p + a.lay.off_x), y = lk_ld_f32(p + a.lay.off_y), z = lk_ld_f32(p + a.lay.off_z);
    const bool blind = a.blind * a.blind > x * x + y * y + z * z;  // blindCheck, lidar_processing.h:96-98
    return ((i % a.filter_num) || blind) ? 0u : 1u;
}
// curvature of the point at p and its message's first / last raw time (t0 / tl: the time fields of the first / last point), per handler
__device__ __forceinline__ float lk_decode_time(const unsigned char* t0, const unsigned char* tl, const unsigned char* p, const LkDecodeArgs& a,
                                                double& first_d, double& last_d) {
    float curv;
    if (a.lay.lidar_type == 3) {  // hesaiHandler: doubles
        first_d = a.time_scale * lk_ld_f64(t0);
        last_d = a.time_scale * lk_ld_f64(tl);
        const double cur = a.time_scale * lk_ld_f64(p + a.lay.off_time);
        curv = (float)(round((cur - first_d) * (double)500.0f) / (double)500.0f);
    } else {
        float first_f, last_f, cur_f;
        if (a.lay.lidar_type == 2) {  // ousterHander: uint32 t
            first_f = (float)(a.time_scale * (double)lk_ld_u32(t0));
            last_f = (float)(a.time_scale * (double)lk_ld_u32(tl));
            cur_f = (float)(a.time_scale * (double)lk_ld_u32(p + a.lay.off_time));
        } else {  // velodyneHandler: float time
            first_f = (float)(a.time_scale * (double)lk_ld_f32(t0));
            last_f = (float)(a.time_scale * (double)lk_ld_f32(tl));
            cur_f = (float)(a.time_scale * (double)lk_ld_f32(p + a.lay.off_time));
        }
        first_d = (double)first_f, last_d = (double)last_f;
        curv = roundf((cur_f - first_f) * 500.0f) / 500.0f;
    }
    return curv;
}

// ---------------------------------------------------------------- the front end over S messages (lk_decode_scan_dev, lk_preprocess_scan_dev: S = 1; lk_decode_scans_dev)
// Decode flags, compaction, scatter, then min/max, cell keys, cell sort, heads, starts, centroids, time sort, gather, over all messages of a
// call at once.  Message s = raw points [pt_off[s], pt_off[s+1]) of the call, its bytes at base + msg_off[s]; the point index of every
// per-point quantity counts from its message's first point.  The decoded points of message s are [dec_off[s], dec_off[s+1]) and carry their
// message id (sid), which keeps bounds, cell keys and cells inside their scan.  ONE message has no tables: pt_off == nullptr means "all n
// points are message 0, at base", sid == nullptr "every point is scan 0" (branches the whole grid takes the same way).
__device__ __forceinline__ int lk_msg_of_point(const unsigned int* __restrict__ pt_off, int S, unsigned int i) {
    int lo = 0, hi = S;   // pt_off[lo] <= i < pt_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pt_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
struct LkMsgPoint {
    int s;                       // the point's message
    unsigned int j, m;           // its index in the message, the message's points
    const unsigned char* bytes;  // the message's first byte
};
__device__ __forceinline__ LkMsgPoint lk_msg_point(const unsigned char* __restrict__ base, const unsigned long long* __restrict__ msg_off,
                                                   const unsigned int* __restrict__ pt_off, int S, unsigned int n, unsigned int i) {
    if (!pt_off) return {0, i, n, base};
    const int s = lk_msg_of_point(pt_off, S, i);
    return {s, i - pt_off[s], pt_off[s + 1] - pt_off[s], base + msg_off[s]};
}
// per point: keep flag
__global__ void __launch_bounds__(256)
    lk_dscan_flags_kernel(const unsigned char* __restrict__ base, const unsigned long long* __restrict__ msg_off, const unsigned int* __restrict__ pt_off,
                          int S, unsigned int n, LkDecodeArgs a, unsigned int* __restrict__ flags) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const LkMsgPoint q = lk_msg_point(base, msg_off, pt_off, S, n, i);
    flags[i] = lk_decode_keep(q.bytes + (size_t)q.j * a.lay.point_step, (int)q.j, a);
}
// scatter the kept points in input order (time arithmetic per handler) with their message id; the first point of a message also writes the
// message's first / last raw time, its first decoded index and the initial bounds / overflow word of its scan
__global__ void __launch_bounds__(256)
    lk_dscan_scatter_kernel(const unsigned char* __restrict__ base, const unsigned long long* __restrict__ msg_off, const unsigned int* __restrict__ pt_off,
                            int S, unsigned int n, LkDecodeArgs a, const unsigned int* __restrict__ flags, const unsigned int* __restrict__ pos,
                            lk_point* __restrict__ out, unsigned int* __restrict__ sid, unsigned int* __restrict__ dec_off, double* __restrict__ first_last,
                            int* __restrict__ mm, unsigned int* __restrict__ err) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const LkMsgPoint q = lk_msg_point(base, msg_off, pt_off, S, n, i);
    const int s = q.s;
    const unsigned char* p = q.bytes + (size_t)q.j * a.lay.point_step;
    double first_d, last_d;
    const float curv = lk_decode_time(q.bytes + a.lay.off_time, q.bytes + (size_t)(q.m - 1) * a.lay.point_step + a.lay.off_time, p, a, first_d, last_d);
    if (q.j == 0) {
        first_last[2 * s] = first_d, first_last[2 * s + 1] = last_d;
        dec_off[s] = pos[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) mm[6 * s + c] = 0x7fffffff, mm[6 * s + 3 + c] = (int)0x80000000;
        err[s] = 0u;
    }
    if (i == n - 1) dec_off[S] = pos[i] + flags[i];
    if (flags[i]) {
        lk_point o;
        o.x = lk_ld_f32(p + a.lay.off_x), o.y = lk_ld_f32(p + a.lay.off_y), o.z = lk_ld_f32(p + a.lay.off_z);
        o.curvature = curv;
        out[pos[i]] = o;
        if (sid) sid[pos[i]] = (unsigned int)s;
    }
}
// per-scan bounds: blockIdx.x = scan, gridDim.y blocks stride over its decoded points
__global__ void __launch_bounds__(256) lk_dscan_minmax_kernel(const lk_point* __restrict__ pts, const unsigned int* __restrict__ dec_off, int* mm) {
    const int s = blockIdx.x;
    const unsigned int e = dec_off[s + 1];
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    for (unsigned int i = dec_off[s] + blockIdx.y * 256u + threadIdx.x; i < e; i += gridDim.y * 256u) {
        const float4 p = reinterpret_cast<const float4*>(pts)[i];
        const int v[3] = {lk_f2ord(p.x), lk_f2ord(p.y), lk_f2ord(p.z)};
#pragma unroll
        for (int c = 0; c < 3; ++c) lo[c] = min(lo[c], v[c]), hi[c] = max(hi[c], v[c]);
    }
    lk_pre_minmax_merge(lo, hi, mm + 6 * s);
}
// cell keys under each scan's own bounds; the scan's first point reports its overflow (PCL refuses this too)
__global__ void __launch_bounds__(256)
    lk_dscan_cellidx_kernel(const lk_point* __restrict__ pts, unsigned int n, float inv, const int* __restrict__ mm, const unsigned int* __restrict__ sid,
                            unsigned int* __restrict__ keys, unsigned int* __restrict__ vals, unsigned int* __restrict__ err) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned int s = sid ? sid[i] : 0u;
    int mn[3], dv[3];
    lk_cell_grid(mm + 6 * s, inv, mn, dv);
    if ((i == 0 || (sid && sid[i - 1] != s)) && lk_cell_overflow(dv)) err[s] = 1u;
    keys[i] = lk_cell_key(reinterpret_cast<const float4*>(pts)[i], inv, mn, dv);
    vals[i] = i;
}
// a cell starts where the sorted key changes, and at every scan boundary as well (equal keys of two scans are two cells)
__global__ void __launch_bounds__(256)
    lk_dscan_heads_kernel(const unsigned int* __restrict__ keys, const unsigned int* __restrict__ sid, unsigned int n, unsigned int* __restrict__ flags) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flags[i] = (i == 0 || keys[i] != keys[i - 1] || (sid && sid[i] != sid[i - 1])) ? 1u : 0u;
}
// first cell of every scan (the rank of its first decoded point among the cell heads) and the total: the scans' CSR offsets over the cells
__global__ void __launch_bounds__(256)
    lk_dscan_celloff_kernel(const unsigned int* __restrict__ dec_off, const unsigned int* __restrict__ pos, const unsigned int* __restrict__ ncells, int S,
                            unsigned int* __restrict__ cell_off) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < S) cell_off[s] = pos[dec_off[s]];
    else if (s == S) cell_off[S] = *ncells;
}

// ---------------------------------------------------------------- time buckets of a batch of scans, found on the device
// KILO.cc:375-378: a bucket is a run of EXACTLY equal curvature inside a time-sorted scan.  For a batch laid out back to back
// (scan s = points [scan_off[s], scan_off[s+1])) the bucket tables of lk_batch_replay_ragged_dev are built here instead of on the
// host: flag the run starts, exclusive-scan the flags, scatter the runs' first indices and times (CSR over all scans).
__device__ __forceinline__ int lk_scan_of_point(const unsigned long long* __restrict__ scan_off, int S, unsigned long long i) {
    int lo = 0, hi = S;   // scan_off[lo] <= i < scan_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (scan_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
__global__ void __launch_bounds__(256)
    lk_rag_flag_kernel(const lk_point* __restrict__ pts, unsigned long long n, const unsigned long long* __restrict__ scan_off, int S,
                       unsigned int* __restrict__ flag, unsigned int* __restrict__ stats) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = lk_scan_of_point(scan_off, S, i);
    const float c = pts[i].curvature;
    const bool head = i == scan_off[s];
    const float cp = head ? c : pts[i - 1].curvature;
    flag[i] = (head || c != cp) ? 1u : 0u;
    if (!(c >= cp) || !isfinite(c)) atomicMax(&stats[3], (unsigned int)(S - s));   // out of time order, NaN or +-inf (an infinite stamp would make the
                                                     // predict's dt infinite): the caller skipped the sort of KILO.cc:367 or handed over a corrupt cloud
}
// stats: [0] total buckets B, [1] largest bucket (points), [2] most buckets in a scan, [3] non-zero: some scan is not sorted by time - S - s of
// the FIRST such scan s (the largest S - s any offending point reports), [4] that scan's index or 0xffffffff (lk_rag_scan_summary_kernel)
__global__ void __launch_bounds__(256)
    lk_rag_scatter_kernel(const lk_point* __restrict__ pts, unsigned long long n, const unsigned long long* __restrict__ scan_off, int S,
                          const unsigned int* __restrict__ flag, const unsigned int* __restrict__ rank, const double* __restrict__ t_begin,
                          unsigned long long* __restrict__ pt_start, double* __restrict__ tb, unsigned int* __restrict__ bstart,
                          unsigned int* __restrict__ stats) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) {
        const int s = lk_scan_of_point(scan_off, S, i);
        const unsigned int g = rank[i];
        pt_start[g] = i;
        tb[g] = t_begin[s] + (double)pts[i].curvature;   // KILO.cc:376
        if (i == scan_off[s]) bstart[s] = g;
    }
    if (i == n - 1) {
        const unsigned int B = rank[i] + flag[i];
        pt_start[B] = n;
        bstart[S] = B;
        stats[0] = B;
    }
}
__global__ void __launch_bounds__(256)
    lk_rag_stats_kernel(const unsigned long long* __restrict__ pt_start, const unsigned int* __restrict__ bstart, int S,
                        unsigned int* __restrict__ stats) {
    const unsigned int B = stats[0];
    const unsigned int g = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256u >= B && blockIdx.x * 256u >= (unsigned int)S) return;
    unsigned int big = g < B ? (unsigned int)(pt_start[g + 1] - pt_start[g]) : 0u;
    unsigned int most = g < (unsigned int)S ? bstart[g + 1] - bstart[g] : 0u;
    for (int m = 32; m; m >>= 1) {   // one atomic per wave, not per bucket
        big = max(big, (unsigned int)__shfl_xor((int)big, m));
        most = max(most, (unsigned int)__shfl_xor((int)most, m));
    }
    if ((threadIdx.x & 63) == 0) {
        if (big) atomicMax(&stats[1], big);
        if (most) atomicMax(&stats[2], most);
    }
}
// Runs of consecutive scans as slots (lk_batch_replay_overlay_runs_dev): run r = the scans run_off[r] .. run_off[r+1), in the CSR tables the contiguous bucket
// range run_b[r] .. run_b[r+1); its start time is its first scan's.  stats[5] = most buckets in a run.
__global__ void __launch_bounds__(256)
    lk_rag_run_tables_kernel(const unsigned int* __restrict__ bstart, const unsigned int* __restrict__ run_off, const double* __restrict__ t0, int R,
                             unsigned int* __restrict__ run_b, double* __restrict__ run_t0, unsigned int* __restrict__ stats) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > R) return;
    const unsigned int b0 = bstart[run_off[r]];
    run_b[r] = b0;
    if (r < R) {
        run_t0[r] = t0[run_off[r]];
        atomicMax(&stats[5], bstart[run_off[r + 1]] - b0);
    }
}
// Per-scan summaries of the CSR tables for a LIVE run (lk_run_scans_dev), where every scan is a launch sequence of its own and the host picks
// the kernel scan by scan: one wave per scan strides over the scan's buckets, wave reductions as above.  sum[s] = { buckets, largest bucket,
// smallest bucket, first message }; nbp[s] = { buckets, 0 }, the pair a stream kernel reads through LkRagged::nb for "a batch of one scan";
// resume[s] = that scan's LkResume (lk_stream.hip: 8 ints), reset, its message cursor at the scan's first message (msg_off: the prefix sum of
// the scans' message counts, or null).  Scan 0's wave also turns stats[3] into the index of the first unsorted scan (stats[4]).
__global__ void __launch_bounds__(256)
    lk_rag_scan_summary_kernel(const unsigned long long* __restrict__ pt_start, const unsigned int* __restrict__ bstart, const unsigned int* __restrict__ msg_off,
                               int S, unsigned int* __restrict__ stats, unsigned int* __restrict__ sum, unsigned int* __restrict__ nbp, int* __restrict__ resume) {
    const int s = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (s >= S) return;   // (wave-uniform)
    const unsigned int b0 = bstart[s], b1 = bstart[s + 1];
    unsigned int big = 0u, small = 0xffffffffu;
    for (unsigned int g = b0 + lane; g < b1; g += LK_WAVE) {
        const unsigned int n = (unsigned int)(pt_start[g + 1] - pt_start[g]);
        big = max(big, n), small = min(small, n);
    }
    for (int m = 32; m; m >>= 1) {
        big = max(big, (unsigned int)__shfl_xor((int)big, m));
        small = min(small, (unsigned int)__shfl_xor((int)small, m));
    }
    if (lane == 0) {
        const unsigned int m0 = msg_off ? msg_off[s] : 0u;
        sum[4 * s] = b1 - b0, sum[4 * s + 1] = big, sum[4 * s + 2] = small, sum[4 * s + 3] = m0;
        nbp[2 * s] = b1 - b0, nbp[2 * s + 1] = 0u;
        if (s == 0) stats[4] = stats[3] ? (unsigned int)S - stats[3] : 0xffffffffu;
    }
    if (lane < 8) resume[8 * s + lane] = lane == 2 ? (int)(msg_off ? msg_off[s] : 0u) : lane == 4 ? -1 : 0;   // { bf, stage1, qi, bi, fb_bucket = -1, 0, 0, 0 }
}

// ---- first frame (KILO.cc:332-352): state initialisation from the first package's messages, cloudLidarToWorld on the raw cloud ----
// StateInitialByImu / StateInitialByKinImu (state_initial.hpp:34-117) as oracle/oracle_kilo.cc's firstFrame restates it: the running mean is
// a serial chain over a few hundred records at most, so lane 0 runs it in plain fp64 (the unit is built with -ffp-contract=off: every
// operation is the reference's own + - * / sqrt) while the block fills P = 1e-6 I.  msgs: n_msg records of `stride` bytes whose acc[3]
// lies at byte acc_off and gyr[3] right behind it (lk_imu: 8, lk_kin_imu: 216).  Literal order: N starts at 1, the mean starts at message 0,
// which the loop then visits again.  cov_acc_ / cov_gyr_ are never read by the reference and are not computed.
__global__ void __launch_bounds__(256)
    lk_ff_init_kernel(LkFilter* __restrict__ f, const unsigned char* __restrict__ msgs, unsigned int n_msg, unsigned int stride, unsigned int acc_off,
                      double gravity, double end_time, double* __restrict__ acc_norm_out) {
    for (int i = threadIdx.x; i < 900; i += 256) f->P[i] = (i / 30 == i % 30) ? 0.000001 : 0.0;
    if (threadIdx.x != 0) return;
    const double* m0 = reinterpret_cast<const double*>(msgs + acc_off);
    double mean[6];   // acc, gyr
    for (int c = 0; c < 6; ++c) mean[c] = m0[c];
    int N = 1;
    for (unsigned int k = 0; k < n_msg; ++k) {
        const double* cur = reinterpret_cast<const double*>(msgs + (size_t)k * stride + acc_off);
        for (int c = 0; c < 6; ++c) mean[c] += (cur[c] - mean[c]) / (double)N;
        N++;
    }
    const double acc_norm = sqrt(mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2]);
    double* x = f->x;
    for (int i = 0; i < LK_STATE_DOUBLES; ++i) x[i] = 0.0;   // a fresh ESKF: everything zero but rot = I (grav is set below)
    x[0] = x[4] = x[8] = 1.0;
    for (int c = 0; c < 3; ++c) {
        x[18 + c] = mean[3 + c];                            // bw_ = mean_gyr
        x[21 + c] = ((-mean[c]) / acc_norm) * gravity;      // grav_ = -mean_acc / acc_norm * gravity: divide, then multiply
    }
    f->last_predict_t = end_time;
    f->last_update_t = end_time;
    *acc_norm_out = acc_norm;
}

// pointLidarToWorld (KILO.cc:89-106) for the raw first cloud under the state lk_ff_init_kernel wrote: widen to fp64, ext_R p + ext_T,
// rot (...) + pos with plain products and sums in the reference's order (no fused multiply-add), cast to float; the body cloud is the raw xyz.
__global__ void __launch_bounds__(256)
    lk_ff_world_kernel(const LkFilter* __restrict__ f, LkParams pr, const lk_point* __restrict__ raw, int n, float* __restrict__ xyz_world,
                       float* __restrict__ xyz_body) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = reinterpret_cast<const float4*>(raw)[i];
    const double l[3] = {(double)p.x, (double)p.y, (double)p.z};
    double b[3], w[3];
    for (int r = 0; r < 3; ++r) b[r] = (pr.ext_R[3 * r] * l[0] + pr.ext_R[3 * r + 1] * l[1] + pr.ext_R[3 * r + 2] * l[2]) + pr.ext_T[r];
    for (int r = 0; r < 3; ++r) w[r] = (f->x[3 * r] * b[0] + f->x[3 * r + 1] * b[1] + f->x[3 * r + 2] * b[2]) + f->x[9 + r];
    for (int r = 0; r < 3; ++r) xyz_world[3 * (size_t)i + r] = (float)w[r];
    xyz_body[3 * (size_t)i] = p.x, xyz_body[3 * (size_t)i + 1] = p.y, xyz_body[3 * (size_t)i + 2] = p.z;
}
