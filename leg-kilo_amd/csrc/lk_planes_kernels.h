// lk_planes_kernels.h - dominant planes peeled off many map clouds by RANSAC (lk_clouds_planes_dev; the arithmetic is lk_planes.h's, shared with the
// host probe).  No cell index is built: a hypothesis is a global model and every record of the remainder is tested against it.  Per call
// lk_c2c_kernels.h's bounds kernel gives the status words, lk_planes_init_kernel the alive words and the labels; then per round, enqueued back to
// back without a readback,
//   lk_prim_exclusive_scan    over the alive words: a record's position in its cloud's remainder is scan[g] - scan[off[c]];
//   lk_planes_compact_kernel  the remainder's records to those positions, so that the sampler's positions index it and the score kernel streams it;
//   lk_planes_score_kernel    the hot one.  A LANE IS A HYPOTHESIS: its first point, u x v and dist^2 |u x v|^2 sit in 14 registers.  A block is
//                             four waves over the same LK_PLANES_GROUP hypotheses and one LK_PLANES_CHUNK records of one cloud's remainder; the
//                             records come through LDS LK_PLANES_TILE at a time as float64, and the four waves take every fourth.  All lanes of
//                             a wave read the same LDS address - a broadcast, no bank conflict.  The grid is (chunks of all clouds, groups):
//                             the chunks are counted from the INPUT sizes on the host, so one huge cloud fills the device as 1 024 small
//                             ones do, and a block whose chunk lies behind the remainder's end returns at once.  A block's counts are added
//                             to score[cloud][h] with atomicAdd: whole numbers, any order gives the same bits;
//   lk_planes_argmax_kernel   one wave per cloud: the largest score, the smallest h among equals; the winner's hypothesis is formed again and
//                             kept for the mark kernel, or the cloud's `done` word is set.  done is written here and read by the NEXT launches;
//   lk_planes_mark_kernel     one thread per record: the winner's test again, the label, the alive word cleared.
// Behind the rounds lk_planes_refit_kernel, one block per (cloud, plane), sums the plane's records in input order - lane-strided partial sums, then a
// fixed tree, lk_sor_stats_kernel's scheme, the centroid first and the centred products second - lk_planes_fit_kernel, one thread per plane, turns the
// sums into the coefficients (lk_eig3.h), and lk_planes_record_kernel writes the cloud's record.  The kept records leave through lk_c2c_kernels.h's compaction tail.  Inside a kernel no thread waits for another workgroup.
// DESIGN.md section 4r says what was measured.
#pragma once
#include "lk_planes.h"
#include "lk_c2c_kernels.h"

struct LkPlanesCall {
    const unsigned int* off;           // [n_clouds + 1], counted from the first record
    const unsigned int* status;        // [n_clouds]
    const unsigned int* chunk_first;   // [n_clouds + 1] score blocks in front of every cloud, ceil(input size / LK_PLANES_CHUNK) each
    const float4* in;                  // the call's first record: input order, [total]
    unsigned int* flag;                // [total + 1] alive words (1: in the remainder), the last one 0; behind the rounds the keep words
    unsigned int* scan;                // [total + 1] their exclusive prefix sum
    float4* rem;                       // [total] the remainders, cloud after cloud
    unsigned int* label;               // [total] input order (the caller's or ours)
    unsigned int* score;               // [n_clouds * n_hyp]
    unsigned int* done;                // [n_clouds]
    unsigned int* n_planes;            // [n_clouds]
    unsigned int* win_h;               // [n_clouds] this round's winner, LK_PLANES_NONE = none
    LkPlanesHyp* win;                  // [n_clouds] its hypothesis
    lk_plane* planes;                  // [n_clouds * max_planes], device
    double* csum;                      // [n_clouds * max_planes * 6] the centred sums xx xy xz yy yz zz of every plane
    lk_planes* out;                    // [n_clouds], device
    LkPlanesAxis axis;
    double dist2;
    unsigned long long seed;
    unsigned int n_clouds, total, n_hyp, max_planes, min_inliers, keep_planes, round;
};

// hypothesis h of this round on the remainder rem[0 .. m)
__device__ __forceinline__ LkPlanesHyp lk_planes_draw(const LkPlanesCall& a, const float4* rem, unsigned int m, unsigned int h) {
    uint32_t i[3];
    lk_planes_sample(a.seed, a.round, h, m, i);
    const float4 p = rem[i[0]], q = rem[i[1]], r = rem[i[2]];
    const float pa[3] = {p.x, p.y, p.z}, pb[3] = {q.x, q.y, q.z}, pc[3] = {r.x, r.y, r.z};
    return lk_planes_hyp(pa, pb, pc, a.dist2, a.axis);
}

__global__ void __launch_bounds__(256) lk_planes_init_kernel(LkPlanesCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.total) return;
    if (g == a.total) {
        a.flag[g] = 0u;
        return;
    }
    a.flag[g] = a.status[lk_c2c_cloud_of(a.off, a.n_clouds, g)] == 0u ? 1u : 0u;
    a.label[g] = LK_PLANES_NONE;
}

__global__ void __launch_bounds__(256) lk_planes_compact_kernel(LkPlanesCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total || !a.flag[g]) return;
    a.rem[a.scan[g]] = a.in[g];
}

__global__ void __launch_bounds__(256) lk_planes_score_kernel(LkPlanesCall a) {
    __shared__ double sx[LK_PLANES_TILE], sy[LK_PLANES_TILE], sz[LK_PLANES_TILE];
    const unsigned int t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned int c = lk_c2c_cloud_of(a.chunk_first, a.n_clouds, blockIdx.x);
    if (a.done[c]) return;   // (every return in front of the barriers is taken by the whole block)
    const unsigned int rb = a.scan[a.off[c]], m = a.scan[a.off[c + 1]] - rb;
    const unsigned int start = (blockIdx.x - a.chunk_first[c]) * LK_PLANES_CHUNK;
    if (!lk_planes_runs(m, a.min_inliers) || start >= m) return;
    const unsigned int end = min(start + LK_PLANES_CHUNK, m);
    const float4* rem = a.rem + rb;
    const unsigned int h = blockIdx.y * LK_PLANES_GROUP + lane;
    LkPlanesHyp hyp = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0};
    if (h < a.n_hyp) hyp = lk_planes_draw(a, rem, m, h);
    unsigned int count = 0u;
    for (unsigned int tile = start; tile < end; tile += LK_PLANES_TILE) {
        __syncthreads();   // the tile before this one has been read
        if (tile + t < end) {
            const float4 p = rem[tile + t];
            sx[t] = p.x, sy[t] = p.y, sz[t] = p.z;
        }
        __syncthreads();
        const unsigned int nt = min(LK_PLANES_TILE, end - tile);
        for (unsigned int k = wave; k < nt; k += 4u) count += lk_planes_inlier(hyp, sx[k], sy[k], sz[k]) ? 1u : 0u;
    }
    if (count) atomicAdd(a.score + (size_t)c * a.n_hyp + h, count);   // (a lane behind n_hyp holds a skipped hypothesis: count 0)
}

__global__ void __launch_bounds__(64) lk_planes_argmax_kernel(LkPlanesCall a) {
    const unsigned int c = blockIdx.x, lane = threadIdx.x;
    const unsigned int rb = a.scan[a.off[c]], m = a.scan[a.off[c + 1]] - rb;
    const bool runs = a.done[c] == 0u && lk_planes_runs(m, a.min_inliers);
    unsigned int best = 0u, best_h = LK_PLANES_NONE;
    if (runs) {
        for (unsigned int h = lane; h < a.n_hyp; h += 64u) {
            const unsigned int s = a.score[(size_t)c * a.n_hyp + h];
            if (lk_planes_better(s, h, best, best_h)) best = s, best_h = h;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int s = __shfl_xor(best, o, 64), sh = __shfl_xor(best_h, o, 64);
        if (sh != LK_PLANES_NONE && lk_planes_better(s, sh, best, best_h)) best = s, best_h = sh;
    }
    if (lane != 0u) return;
    if (!runs || best < a.min_inliers) {
        a.done[c] = 1u, a.win_h[c] = LK_PLANES_NONE;
        return;
    }
    a.win_h[c] = best_h, a.win[c] = lk_planes_draw(a, a.rem + rb, m, best_h);
    lk_plane* pl = a.planes + (size_t)c * a.max_planes + a.round;
    pl->n_inliers = best, pl->hyp = best_h;
    a.n_planes[c] = a.round + 1u;
}

__global__ void __launch_bounds__(256) lk_planes_mark_kernel(LkPlanesCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total || !a.flag[g]) return;
    const unsigned int c = lk_c2c_cloud_of(a.off, a.n_clouds, g);
    if (a.win_h[c] == LK_PLANES_NONE) return;
    const float4 p = a.in[g];
    if (lk_planes_inlier(a.win[c], p.x, p.y, p.z)) a.flag[g] = 0u, a.label[g] = a.round;
}

// blockIdx.x = cloud, blockIdx.y = plane.  Lane t takes the cloud's records t, t + 256, ... in ascending order, then the 256 partial sums meet in a
// fixed tree: the order depends on the cloud and its labels alone
template <int ROWS>
__device__ __forceinline__ void lk_planes_tree(double (*sh)[256], unsigned int t) {
    __syncthreads();
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < ROWS; ++k) sh[k][t] = sh[k][t] + sh[k][t + o];
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) lk_planes_refit_kernel(LkPlanesCall a) {
    __shared__ double sh[6][256];
    __shared__ unsigned int cnt[256];
    const unsigned int c = blockIdx.x, r = blockIdx.y, t = threadIdx.x, b = a.off[c], n = a.off[c + 1] - b;
    if (r >= a.n_planes[c]) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    unsigned int k = 0u;
    for (unsigned int i = t; i < n; i += 256u) {
        if (a.label[b + i] != r) continue;
        const float4 p = a.in[b + i];
        sx = sx + (double)p.x, sy = sy + (double)p.y, sz = sz + (double)p.z, k += 1u;
    }
    sh[0][t] = sx, sh[1][t] = sy, sh[2][t] = sz, cnt[t] = k;
    lk_planes_tree<3>(sh, t);
    for (unsigned int o = 128; o > 0; o >>= 1) {
        if (t < o) cnt[t] += cnt[t + o];
        __syncthreads();
    }
    const unsigned int ni = cnt[0];
    const double cx = sh[0][0] / (double)ni, cy = sh[1][0] / (double)ni, cz = sh[2][0] / (double)ni;
    __syncthreads();
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (unsigned int i = t; i < n; i += 256u) {
        if (a.label[b + i] != r) continue;
        const float4 p = a.in[b + i];
        const double dx = (double)p.x - cx, dy = (double)p.y - cy, dz = (double)p.z - cz;
        xx = xx + dx * dx, xy = xy + dx * dy, xz = xz + dx * dz, yy = yy + dy * dy, yz = yz + dy * dz, zz = zz + dz * dz;
    }
    sh[0][t] = xx, sh[1][t] = xy, sh[2][t] = xz, sh[3][t] = yy, sh[4][t] = yz, sh[5][t] = zz;
    lk_planes_tree<6>(sh, t);
    if (t != 0u) return;
    lk_plane* pl = a.planes + (size_t)c * a.max_planes + r;
    pl->centroid[0] = cx, pl->centroid[1] = cy, pl->centroid[2] = cz;
#pragma unroll
    for (int j = 0; j < 6; ++j) a.csum[((size_t)c * a.max_planes + r) * 6 + j] = sh[j][0];
}
// one thread per (cloud, plane): lk_eig3.h over the sums.  (Its acos and cos are the device library's, whose argument reduction keeps a table in
// scratch: 48 bytes a lane here as in every kernel that includes lk_eig3.h.  That is why this is not the refit kernel's last step.)
__global__ void __launch_bounds__(256) lk_planes_fit_kernel(LkPlanesCall a) {
    const size_t g = blockIdx.x * 256ull + threadIdx.x;
    if (g >= (size_t)a.n_clouds * a.max_planes || g % a.max_planes >= a.n_planes[g / a.max_planes]) return;
    lk_plane* pl = a.planes + g;
    const double cen[3] = {pl->centroid[0], pl->centroid[1], pl->centroid[2]};
    const double cs[6] = {a.csum[6 * g], a.csum[6 * g + 1], a.csum[6 * g + 2], a.csum[6 * g + 3], a.csum[6 * g + 4], a.csum[6 * g + 5]};
    LkPlanesFit f;
    lk_planes_fit(cen, cs, pl->n_inliers, a.axis, &f);
#pragma unroll
    for (int j = 0; j < 3; ++j) pl->normal[j] = f.normal[j], pl->eig[j] = f.eig[j];
    pl->d = f.d, pl->rmse = f.rmse;
}

// the cloud's record, and the alive words turned into the keep words
__global__ void __launch_bounds__(256) lk_planes_record_kernel(LkPlanesCall a) {
    const unsigned int c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.n_clouds) return;
    const unsigned int st = a.status[c], np = a.n_planes[c];
    const unsigned long long n = a.off[c + 1] - a.off[c];
    unsigned long long on = 0ull;
    for (unsigned int r = 0; r < np; ++r) on += a.planes[(size_t)c * a.max_planes + r].n_inliers;
    lk_planes o;
    o.n_points = n, o.n_on_planes = on, o.n_rest = st ? 0ull : n - on, o.n_kept = a.keep_planes ? on : o.n_rest;
    o.n_planes = np, o.status = st;
#pragma unroll
    for (int k = 0; k < 6; ++k) o.pad[k] = 0u;
    a.out[c] = o;
}
__global__ void __launch_bounds__(256) lk_planes_keep_kernel(LkPlanesCall a) {
    const unsigned int g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.total) return;
    if (a.keep_planes) a.flag[g] = a.label[g] != LK_PLANES_NONE ? 1u : 0u;   // (otherwise the remainder: the alive words as they are)
}
