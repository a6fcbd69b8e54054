// Per-region moments of B estimates (and of their error against a full-dose target) over a region index: a sorted
// voxel-index list in CSR form (definitions in include/ddpm3d.h).  Region r's entries are cut into
// consecutive chunks of DDPM3D_ROI_CHUNK; one workgroup per (chunk, estimate) gathers its values, reduces them in a
// fixed order and writes one fp64 record to the caller's workspace; a second launch folds each (estimate, region)'s
// records in a fixed order.  No atomics: the same bits on every run, and row b does not depend on B.  The reduction
// is record_reduce.h's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "record_reduce.h"

namespace {

constexpr int ROI_THREADS = 256;
constexpr int ROI_PER = DDPM3D_ROI_CHUNK / ROI_THREADS;      // entries per thread and chunk
constexpr int ROI_REC = DDPM3D_ROI_REC;
static_assert(DDPM3D_ROI_CHUNK % ROI_THREADS == 0, "a chunk is a whole number of passes");

// sums but for the minimum and the maximum of x
struct RoiCols {
    static constexpr int COLS = ROI_REC, REC = ROI_REC;
    static constexpr RrOp op(int k) { return k == DDPM3D_ROI_MIN_X ? RR_MIN : k == DDPM3D_ROI_MAX_X ? RR_MAX : RR_SUM; }
};

// Workgroup (c, b): chunk c of the index belongs to the region r with chunks[r] <= c < chunks[r + 1] (a search of
// the prefix table; empty regions own no chunk) and covers entries [e0, e1) of it.  A thread takes entries
// e0 + tid + 256 j, j ascending: all its index loads are issued first, then all gathers, then the fp64 terms.
__global__ __launch_bounds__(ROI_THREADS) void roi_chunk_kernel(
    const float* __restrict__ est, const float* __restrict__ target, int64_t voxels, int R,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ chunks, const int64_t* __restrict__ index,
    int64_t total, double* __restrict__ ws) {
    // x * x is exact in fp64; e * e and the sums must round one at a time (no v_fma_f64), as the reference forms them
#pragma clang fp contract(off)
    const int64_t c = blockIdx.x;
    const int b = blockIdx.y;
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunks[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t e0 = offsets[lo] + (c - chunks[lo]) * DDPM3D_ROI_CHUNK;
    const int64_t end = offsets[lo + 1];
    const int64_t e1 = e0 + DDPM3D_ROI_CHUNK < end ? e0 + DDPM3D_ROI_CHUNK : end;
    const float* __restrict__ xb = est + (int64_t)b * voxels;

    int64_t at[ROI_PER];
#pragma unroll
    for (int j = 0; j < ROI_PER; ++j) {
        const int64_t e = e0 + threadIdx.x + j * ROI_THREADS;
        at[j] = e < e1 ? index[e] : -1;
    }
    float x[ROI_PER], y[ROI_PER];
#pragma unroll
    for (int j = 0; j < ROI_PER; ++j) {
        x[j] = at[j] >= 0 ? xb[at[j]] : 0.0f;
        y[j] = (target && at[j] >= 0) ? target[at[j]] : 0.0f;
    }
    double sx = 0.0, sxx = 0.0, se = 0.0, sa = 0.0, sq = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    unsigned n = 0;
#pragma unroll
    for (int j = 0; j < ROI_PER; ++j) {
        if (at[j] < 0) continue;
        const double xd = (double)x[j];
        n += 1;
        sx += xd;
        sxx += xd * xd;
        mn = fminf(mn, x[j]);
        mx = fmaxf(mx, x[j]);
        if (target) {
            const double e = xd - (double)y[j];
            se += e;
            sa += fabs(e);
            sq += e * e;
        }
    }
    double rec[ROI_REC];
    rec[DDPM3D_ROI_N] = (double)n;
    rec[DDPM3D_ROI_SUM_X] = sx;
    rec[DDPM3D_ROI_SUM_SQ_X] = sxx;
    rec[DDPM3D_ROI_MIN_X] = (double)mn;
    rec[DDPM3D_ROI_MAX_X] = (double)mx;
    rec[DDPM3D_ROI_SUM_E] = se;
    rec[DDPM3D_ROI_SUM_ABS_E] = sa;
    rec[DDPM3D_ROI_SUM_SQ_E] = sq;
    rr_write_record<RoiCols, ROI_THREADS>(rec, ws + ((int64_t)b * total + c) * ROI_REC);
}

// Workgroup (r, b): region r's records of estimate b, chunk p to thread p mod 256 in ascending p, then the
// workgroup's fold.  A region without a chunk gets N = 0, sums 0, MIN = +inf, MAX = -inf.
__global__ __launch_bounds__(ROI_THREADS) void roi_fold_kernel(const double* __restrict__ ws,
                                                               const int64_t* __restrict__ chunks, int64_t total,
                                                               int R, double* __restrict__ out) {
    const int r = blockIdx.x, b = blockIdx.y;
    const int64_t c0 = chunks[r], c1 = chunks[r + 1];
    rr_fold_record<RoiCols, ROI_THREADS>(ws + ((int64_t)b * total + c0) * ROI_REC, c1 - c0,
                                         out + ((int64_t)b * R + r) * ROI_REC);
}

}  // namespace

hipError_t ddpm3d_launch_roi_moments(const float* est, const float* target, int B, int64_t voxels,
                                     const ddpm3d_roi_index& ix, int64_t chunks, double* ws, double* out,
                                     hipStream_t st) {
    if (chunks > 0) {
        hipLaunchKernelGGL(roi_chunk_kernel, dim3((unsigned)chunks, B), dim3(ROI_THREADS), 0, st, est, target, voxels,
                           ix.regions, ix.d_offsets, ix.d_chunks, ix.d_index, chunks, ws);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(roi_fold_kernel, dim3(ix.regions, B), dim3(ROI_THREADS), 0, st, ws, ix.d_chunks, chunks,
                       ix.regions, out);
    return hipGetLastError();
}
