// lk_mapcloud_kernels.h - the back end's voxel grid (lk_downsample_clouds_dev): PcdSaver::downsampleAndSave (common/pcd_saver.hpp:114-121) over many
// files at once.  File f = the registered points [file_off[f], file_off[f+1]) of one buffer of 16-byte x y z intensity records; per file the definition
// is the front end's (oracle/preprocess_oracle.py::voxel_grid_centroid, intensity in the place of curvature) and so is the cell arithmetic: lk_f2ord,
// lk_cell_grid, lk_cell_key and lk_cell_overflow of lk_pre_kernels.h.  What differs from lk_dscan_*: bounds, keys and cells stay inside a FILE, a file
// whose grid overflows an int comes out unfiltered (pcl::VoxelGrid's answer; its points get their index in the file as key, so every point is a cell
// of its own, in input order), and a cell may hold hundreds of points (a robot that stands still), so the centroid kernel reads records that a gather
// has put into cell order instead of chasing the sort's indices.
// Streaming kernels, 256 threads, one record per lane.  HBM traffic per point: bounds 16 B, keys 16 + 8, sort 8 + 8 per
// pass (counted as one), heads 4 + 4, scan 4 + 4, starts 8, gather 4 + 16 + 16, centroid 16 = 132 B; per cell 4 + 4 (its start) + 16 (its record) = 24 B.
#pragma once
#include "lk_pre_kernels.h"

#define LK_MC_BAD_NONFINITE 1   // status word of a file: a coordinate that is NaN or +-inf
#define LK_MC_BAD_RANGE 2       //                        |p * inv| >= 2^30 (floor(p * inv) and the divisions stay inside an int below that)

// per file: { min_b[3], div_b[3], unfiltered, status }
#define LK_MC_GRID_WORDS 8

__global__ void __launch_bounds__(256) lk_mc_init_kernel(int* __restrict__ mm, unsigned int* __restrict__ status, int F) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) mm[6 * f + c] = 0x7fffffff, mm[6 * f + 3 + c] = (int)0x80000000;
    status[f] = 0u;
}
// per-file bounds: blockIdx.x = file, gridDim.y blocks stride over its points; the same pass raises the file's non-finite / range bits
__global__ void __launch_bounds__(256)
    lk_mc_bounds_kernel(const float4* __restrict__ pts, const unsigned int* __restrict__ file_off, float inv, int* mm, unsigned int* status) {
    const int f = blockIdx.x;
    const unsigned int e = file_off[f + 1];
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    unsigned int bad = 0u;
    for (unsigned int i = file_off[f] + blockIdx.y * 256u + threadIdx.x; i < e; i += gridDim.y * 256u) {
        const float4 p = pts[i];
        const float q[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!isfinite(q[c])) bad |= LK_MC_BAD_NONFINITE;
            else if (!(fabsf(q[c] * inv) < 1073741824.0f)) bad |= LK_MC_BAD_RANGE;
            const int v = lk_f2ord(q[c]);
            lo[c] = min(lo[c], v), hi[c] = max(hi[c], v);
        }
    }
    if (bad) atomicOr(&status[f], bad);   // (rare; nobody leaves early: the merge below has a barrier)
    lk_pre_minmax_merge(lo, hi, mm + 6 * f);
}
// per file: its grid under the front end's arithmetic, whether that grid overflows (the file then comes out unfiltered), its status
__global__ void __launch_bounds__(256)
    lk_mc_grid_kernel(const int* __restrict__ mm, const unsigned int* __restrict__ status, float inv, int F, int* __restrict__ grid) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int mn[3] = {0, 0, 0}, dv[3] = {1, 1, 1};
    const unsigned int st = status[f];
    if (st == 0u) lk_cell_grid(mm + 6 * f, inv, mn, dv);   // (a refused file's bounds do not convert to int)
    int* g = grid + LK_MC_GRID_WORDS * f;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = mn[c], g[3 + c] = dv[c];
    g[6] = (st == 0u && lk_cell_overflow(dv)) ? 1 : 0;
    g[7] = (int)st;
}
// cell key of every point under its file's grid (the file is found by bisection in file_off); an unfiltered file's points: their index in the file
__global__ void __launch_bounds__(256)
    lk_mc_keys_kernel(const float4* __restrict__ pts, unsigned int n, const unsigned int* __restrict__ file_off, int F, float inv, const int* __restrict__ grid,
                      unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int f = lk_msg_of_point(file_off, F, i);
    const int* g = grid + LK_MC_GRID_WORDS * f;
    const int mn[3] = {g[0], g[1], g[2]}, dv[3] = {g[3], g[4], g[5]};
    keys[i] = g[6] ? i - file_off[f] : lk_cell_key(pts[i], inv, mn, dv);
    vals[i] = i;
}
// a new cell at every key change and at every file's first point (equal keys of two files are two cells)
__global__ void __launch_bounds__(256)
    lk_mc_heads_kernel(const unsigned int* __restrict__ keys, unsigned int n, const unsigned int* __restrict__ file_off, int F, unsigned int* __restrict__ flags) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    unsigned int head = (i == 0u || keys[i] != keys[i - 1]) ? 1u : 0u;
    if (!head) head = file_off[lk_msg_of_point(file_off, F, i)] == i ? 1u : 0u;
    flags[i] = head;
}
// the records in cell order: neighbouring lanes write neighbouring 16-byte records, and the centroid kernel reads them the same way
__global__ void __launch_bounds__(256)
    lk_mc_gather_kernel(const float4* __restrict__ pts, const unsigned int* __restrict__ order, unsigned int n, float4* __restrict__ sorted) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) sorted[i] = pts[order[i]];
}
// one thread per cell over the gathered records: sequential float32 sums in input order (the sort is stable), divided by the float count.  A cell of an
// unfiltered file is its one point as it came (0.0f + x would turn -0.0f into 0.0f).
__global__ void __launch_bounds__(256)
    lk_mc_centroid_kernel(const float4* __restrict__ sorted, const int* __restrict__ starts, const unsigned int* __restrict__ ncells_p, unsigned int n,
                          const unsigned int* __restrict__ file_off, int F, const int* __restrict__ grid, float4* __restrict__ out) {
    const unsigned int c = blockIdx.x * 256u + threadIdx.x;
    const unsigned int ncells = *ncells_p;
    if (c >= ncells) return;
    const unsigned int b = (unsigned int)starts[c], e = (c + 1 < ncells) ? (unsigned int)starts[c + 1] : n;
    if (e - b == 1u && grid[LK_MC_GRID_WORDS * lk_msg_of_point(file_off, F, b) + 6]) {
        out[c] = sorted[b];
        return;
    }
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
    for (unsigned int k = b; k < e; ++k) {
        const float4 p = sorted[k];
        sx = sx + p.x, sy = sy + p.y, sz = sz + p.z, sw = sw + p.w;
    }
    const float cnt = (float)(e - b);
    out[c] = make_float4(sx / cnt, sy / cnt, sz / cnt, sw / cnt);
}
