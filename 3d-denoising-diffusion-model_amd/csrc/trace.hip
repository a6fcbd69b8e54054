// Per-step convergence trace of a sampling loop (definitions in include/ddpm3d.h): weighted moments
// of B estimates (one step's pred_xstart) against their targets and against the previous step's estimate.  The
// shape is metrics.hip's error-moments pair: workgroup (part, b) reduces one chunk of estimate b in a fixed order
// and writes one fp64 record to the caller's workspace, a second, small launch folds a sample's records in a fixed
// order.  No atomics: the same bits on every run, and the plan depends on `voxels` alone, so row b of a batch carries
// the bits of a call on estimate b.  Offsets are 64-bit.  The reduction is record_reduce.h's, every column a sum.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "record_reduce.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_VEC = 4;
constexpr int TR_MAX_PARTS = 2048;         // 8 workgroups per CU: enough loads in flight to stream from HBM
constexpr int TR_REC = DDPM3D_TR_REC;

using TrCols = RrSum<TR_REC>;

template <int V>
__device__ __forceinline__ void tr_load(const float* __restrict__ p, int64_t i, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = p[i];
    }
}

// Workgroup (part, b) reduces voxels [part * chunk, (part + 1) * chunk) of estimate b; chunk is a multiple of
// TR_THREADS * TR_VEC.  V = 4: one 16-byte load per thread, pass and input.  A voxel whose weight is not above 0
// is skipped before any of its values enters a term: what est, prev or target hold there (NaN included) is never
// added.  prev, target and weight may be NULL; tstride / wstride are 0 (shared) or voxels (one per estimate).
template <int V>
__global__ __launch_bounds__(TR_THREADS) void trace_moments_kernel(
    const float* __restrict__ est, const float* __restrict__ prev, const float* __restrict__ target,
    const float* __restrict__ weight, int64_t voxels, int64_t tstride, int64_t wstride, int64_t chunk, int parts,
    double* __restrict__ ws) {
    // every product and every sum rounds on its own (no v_fma_f64), as the yardstick forms them
#pragma clang fp contract(off)
    const int part = blockIdx.x, b = blockIdx.y;
    const int64_t v0 = (int64_t)part * chunk;
    const int64_t v1 = v0 + chunk < voxels ? v0 + chunk : voxels;
    const float* __restrict__ xb = est + (int64_t)b * voxels;
    const float* __restrict__ pb = prev ? prev + (int64_t)b * voxels : nullptr;
    const float* __restrict__ yb = target ? target + (int64_t)b * tstride : nullptr;
    const float* __restrict__ wb = weight ? weight + (int64_t)b * wstride : nullptr;
    double sw = 0.0, se = 0.0, sa = 0.0, sq = 0.0, syy = 0.0, sx = 0.0, sxx = 0.0, sdd = 0.0, sc = 0.0;
    unsigned n = 0;                       // at most chunk / TR_THREADS * V counts per thread: below 2^32
    for (int64_t i0 = v0 + (int64_t)threadIdx.x * V; i0 < v1; i0 += TR_THREADS * V) {
        float x[V], p[V], y[V], w[V];
        tr_load<V>(xb, i0, x);
        if (pb) tr_load<V>(pb, i0, p);
        if (yb) tr_load<V>(yb, i0, y);
        if (wb) tr_load<V>(wb, i0, w);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (wb && !(w[v] > 0.0f)) continue;
            const double wd = wb ? (double)w[v] : 1.0;
            const double xd = (double)x[v];
            n += 1;
            sw += wd;
            sx += wd * xd;
            sxx += wd * (xd * xd);
            if (fabs(xd) >= 1.0) sc += wd;
            if (yb) {
                const double yd = (double)y[v];
                const double e = xd - yd;
                se += wd * e;
                sa += wd * fabs(e);
                sq += wd * (e * e);
                syy += wd * (yd * yd);
            }
            if (pb) {
                const double d = xd - (double)p[v];
                sdd += wd * (d * d);
            }
        }
    }
    double rec[TR_REC];
    rec[DDPM3D_TR_W] = sw;
    rec[DDPM3D_TR_N] = (double)n;
    rec[DDPM3D_TR_SUM_E] = se;
    rec[DDPM3D_TR_SUM_ABS_E] = sa;
    rec[DDPM3D_TR_SUM_SQ_E] = sq;
    rec[DDPM3D_TR_SUM_SQ_Y] = syy;
    rec[DDPM3D_TR_SUM_X] = sx;
    rec[DDPM3D_TR_SUM_SQ_X] = sxx;
    rec[DDPM3D_TR_SUM_SQ_D] = sdd;
    rec[DDPM3D_TR_CLIPPED] = sc;
    rr_write_record<TrCols, TR_THREADS>(rec, ws + ((size_t)b * parts + part) * TR_REC);
}

// One workgroup per estimate: its records in a fixed order.
__global__ __launch_bounds__(TR_THREADS) void trace_moments_fold_kernel(const double* __restrict__ ws, int parts,
                                                                        double* __restrict__ out) {
    const int b = blockIdx.x;
    rr_fold_record<TrCols, TR_THREADS>(ws + (size_t)b * parts * TR_REC, parts, out + (size_t)b * TR_REC);
}

}  // namespace

size_t ddpm3d_tr_workspace_bytes(int B, int64_t voxels) {
    return rr_workspace_bytes(B, voxels, TR_THREADS * TR_VEC, TR_MAX_PARTS, TR_REC);
}

hipError_t ddpm3d_launch_trace_moments(const float* est, const float* prev, const float* target, const float* weight,
                                       int B, int64_t voxels, int64_t target_stride, int64_t weight_stride, double* ws,
                                       double* out, hipStream_t st) {
    const RrPlan p = rr_plan(voxels, TR_THREADS * TR_VEC, TR_MAX_PARTS);
    // every row of every input starts a multiple of `voxels` floats behind its base: one test per pointer
    const bool wide = voxels % TR_VEC == 0 && aligned(est, 16) && (!prev || aligned(prev, 16)) &&
                      (!target || aligned(target, 16)) && (!weight || aligned(weight, 16));
    const dim3 grid(p.parts, B);
    if (wide)
        hipLaunchKernelGGL(trace_moments_kernel<TR_VEC>, grid, dim3(TR_THREADS), 0, st, est, prev, target, weight,
                           voxels, target_stride, weight_stride, p.chunk, p.parts, ws);
    else
        hipLaunchKernelGGL(trace_moments_kernel<1>, grid, dim3(TR_THREADS), 0, st, est, prev, target, weight, voxels,
                           target_stride, weight_stride, p.chunk, p.parts, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(trace_moments_fold_kernel, dim3(B), dim3(TR_THREADS), 0, st, ws, p.parts, out);
    return hipGetLastError();
}
