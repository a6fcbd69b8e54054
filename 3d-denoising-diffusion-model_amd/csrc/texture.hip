// Per-region grey-level co-occurrence matrices (GLCM) and grey-level histograms of B estimates over a region index
// (definitions in include/ddpm3d.h).  The decomposition is roi.hip's: region r's entries are cut into
// consecutive chunks of DDPM3D_ROI_CHUNK, and a workgroup serves TEX_SPAN consecutive chunks of one region for one
// estimate.  Its matrix and histogram live in LDS as 32-bit counters; a thread walks entries of the index, decodes
// (z, y, x), and for each of the 13 direction vectors tests the neighbour's coordinates against the extents before
// any load, compares region_of, bins the neighbour's value and adds to both cells with LDS atomics.  A pair is found
// from its lower voxel only (every direction vector points to a higher flat index), so chunk borders need no care.
// At its end the workgroup adds its non-zero cells to the 64-bit counters in global memory.  Integer atomics only:
// the sums do not depend on the order they resolve in, so the output is the same bits on every run and for every
// launch geometry, and row b does not depend on B.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

// Chunks of one region a workgroup keeps its LDS matrix across (nothing in the result depends on it).  The grid stays
// one workgroup per chunk and the span's first one does the work, so a span that shares a factor with the number of
// XCDs (8; workgroups go to them round-robin) leaves the work of a large region on a part of the chip.  1 is what
// measured best: the flush is about a tenth of the launch.
#ifndef DDPM3D_TEX_SPAN
#define DDPM3D_TEX_SPAN 1
#endif

namespace {

constexpr int TEX_THREADS = 256;
constexpr int TEX_L = DDPM3D_TEX_MAX_LEVELS;
constexpr int TEX_SPAN = DDPM3D_TEX_SPAN;
constexpr int TEX_DIRS = 13;
// a 32-bit LDS cell gains at most 26 per entry
static_assert((int64_t)TEX_SPAN * DDPM3D_ROI_CHUNK * 26 < ((int64_t)1 << 32), "an LDS counter must not wrap");
static_assert(TEX_SPAN >= 1, "a workgroup serves at least one chunk");

typedef unsigned long long u64;

// the grey level of t = (x - lo) * inv_w; *edge is 1 below the first bin, 2 at or above the last bin's end, else 0.
// The comparisons are made on the float so that no out-of-range value is ever converted.
__device__ __forceinline__ int tex_level(float t, int levels, int* edge) {
    const float f = floorf(t);
    if (f < 0.0f) { *edge = 1; return 0; }
    if (f >= (float)levels) { *edge = 2; return levels - 1; }
    *edge = 0;
    return (int)f;
}

__global__ __launch_bounds__(TEX_THREADS) void roi_texture_kernel(
    const float* __restrict__ est, const int16_t* __restrict__ region_of, int D, int H, int W, int R,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ chunks, const int64_t* __restrict__ index,
    const float* __restrict__ lo_all, const float* __restrict__ inv_all, int levels, u64* __restrict__ glcm,
    u64* __restrict__ hist, u64* __restrict__ counts) {
    // the subtraction and the product round to fp32 one at a time
#pragma clang fp contract(off)
    __shared__ unsigned s_c[TEX_L * TEX_L];
    __shared__ unsigned s_h[TEX_L];
    __shared__ unsigned s_n[DDPM3D_TEX_REC];

    const int64_t c = blockIdx.x;
    const int b = blockIdx.y;
    int r = 0, hi = R;
    while (hi - r > 1) {
        const int mid = (r + hi) >> 1;
        if (chunks[mid] <= c) r = mid; else hi = mid;
    }
    const int64_t first = c - chunks[r];
    if (first % TEX_SPAN != 0) return;               // the whole workgroup: the span's first chunk does the work
    const int64_t e0 = offsets[r] + first * DDPM3D_ROI_CHUNK;
    const int64_t end = offsets[r + 1];
    const int64_t e1 = e0 + (int64_t)TEX_SPAN * DDPM3D_ROI_CHUNK < end ? e0 + (int64_t)TEX_SPAN * DDPM3D_ROI_CHUNK : end;

    const int cells = levels * levels;
    for (int i = threadIdx.x; i < cells; i += TEX_THREADS) s_c[i] = 0u;
    if (threadIdx.x < TEX_L) s_h[threadIdx.x] = 0u;
    if (threadIdx.x < DDPM3D_TEX_REC) s_n[threadIdx.x] = 0u;
    __syncthreads();

    const int HW = H * W;
    const int voxels = D * HW;                       // at most 2^31 - 1 (the entry has checked)
    const float* __restrict__ xb = est + (int64_t)b * voxels;
    const float lo = lo_all[(int64_t)b * R + r];
    const float inv_w = inv_all[(int64_t)b * R + r];
    const int16_t mine = (int16_t)(r + 1);
    unsigned n = 0, below = 0, above = 0, pairs = 0;

    for (int64_t e = e0 + threadIdx.x; e < e1; e += TEX_THREADS) {
        const int64_t at = index[e];
        if (at < 0 || at >= voxels) continue;        // the producer guarantees it; no load leaves the volume regardless
        const int v = (int)at;
        const float tv = (xb[v] - lo) * inv_w;
        if (tv != tv) continue;                      // NaN: the voxel is not counted at all
        int edge;
        const int gv = tex_level(tv, levels, &edge);
        n += 1;
        below += edge == 1;
        above += edge == 2;
        atomicAdd(&s_h[gv], 1u);
        const int z = v / HW, rem = v - z * HW;
        const int y = rem / W, x = rem - y * W;

        // the 13 offsets (dz, dy, dx) lexicographically above (0, 0, 0): first every region_of load, then every value
        int nb[TEX_DIRS];
#pragma unroll
        for (int k = 0; k < TEX_DIRS; ++k) {
            const int q = k + 14;                    // (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), above the centre's 13
            const int dz = q / 9 - 1, dy = (q / 3) % 3 - 1, dx = q % 3 - 1;
            const int nz = z + dz, ny = y + dy, nx = x + dx;
            const bool in = nz < D && ny >= 0 && ny < H && nx >= 0 && nx < W;      // dz >= 0, so nz >= 0
            const int u = v + dz * HW + dy * W + dx;
            nb[k] = (in && region_of[u] == mine) ? u : -1;
        }
        float xn[TEX_DIRS];
#pragma unroll
        for (int k = 0; k < TEX_DIRS; ++k) xn[k] = nb[k] >= 0 ? xb[nb[k]] : 0.0f;
#pragma unroll
        for (int k = 0; k < TEX_DIRS; ++k) {
            if (nb[k] < 0) continue;
            const float tu = (xn[k] - lo) * inv_w;
            if (tu != tu) continue;
            int unused;
            const int gu = tex_level(tu, levels, &unused);
            pairs += 1;
            if (gu == gv) {
                atomicAdd(&s_c[gv * levels + gv], 2u);
            } else {
                atomicAdd(&s_c[gv * levels + gu], 1u);
                atomicAdd(&s_c[gu * levels + gv], 1u);
            }
        }
    }
    if (n) atomicAdd(&s_n[DDPM3D_TEX_N], n);
    if (below) atomicAdd(&s_n[DDPM3D_TEX_BELOW], below);
    if (above) atomicAdd(&s_n[DDPM3D_TEX_ABOVE], above);
    if (pairs) atomicAdd(&s_n[DDPM3D_TEX_PAIRS], pairs);
    __syncthreads();

    const int64_t br = (int64_t)b * R + r;
    u64* __restrict__ g_c = glcm + br * cells;
    for (int i = threadIdx.x; i < cells; i += TEX_THREADS) {
        const unsigned add = s_c[i];
        if (add) atomicAdd(&g_c[i], (u64)add);
    }
    if (threadIdx.x < levels) {
        const unsigned add = s_h[threadIdx.x];
        if (add) atomicAdd(&hist[br * levels + threadIdx.x], (u64)add);
    }
    if (threadIdx.x < DDPM3D_TEX_REC) {
        const unsigned add = s_n[threadIdx.x];
        if (add) atomicAdd(&counts[br * DDPM3D_TEX_REC + threadIdx.x], (u64)add);
    }
}

}  // namespace

hipError_t ddpm3d_launch_roi_texture(const float* est, int B, int D, int H, int W, const ddpm3d_roi_index& ix,
                                     int64_t chunks, const int16_t* region_of, const float* lo, const float* inv_w,
                                     int levels, uint64_t* glcm, uint64_t* hist, uint64_t* counts, hipStream_t st) {
    const size_t br = (size_t)B * ix.regions;
    hipError_t e = hipMemsetAsync(glcm, 0, br * levels * levels * sizeof(uint64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(hist, 0, br * levels * sizeof(uint64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, br * DDPM3D_TEX_REC * sizeof(uint64_t), st);
    if (e != hipSuccess || chunks == 0) return e;
    hipLaunchKernelGGL(roi_texture_kernel, dim3((unsigned)chunks, B), dim3(TEX_THREADS), 0, st, est, region_of, D, H,
                       W, ix.regions, ix.d_offsets, ix.d_chunks, ix.d_index, lo, inv_w, levels, (u64*)glcm, (u64*)hist,
                       (u64*)counts);
    return hipGetLastError();
}
