// Image-quality metrics of an estimate against a full-dose target volume (definitions in
// include/ddpm3d.h).  Both entries reduce B estimates against one shared target in one launch plus a fold:
// every workgroup writes one fp64 record to the caller's workspace and a second, small launch folds a volume's
// records in a fixed order.  No floating-point atomics: the same bits on every run.  Offsets are 64-bit
// (B * voxels passes 2^31 for 16 whole-body draws).  The reduction is record_reduce.h's; records are written with
// 4-byte stores (halves of the doubles), the map with one float per lane: no wide store whose data registers could be
// rewritten behind it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "record_reduce.h"
#include "ssim3d_body.h"

namespace {

// ------------------------------------------------------------------------------------------- error moments
constexpr int EM_THREADS = 256;
constexpr int EM_VEC = 4;
constexpr int EM_MAX_PARTS = 2048;         // 8 workgroups per CU: enough loads in flight to stream from HBM
constexpr int EM_REC = DDPM3D_EM_REC;

// sums in columns 0..5 and 8..9, min / max in 6 / 7
struct EmCols {
    static constexpr int COLS = EM_REC, REC = EM_REC;
    static constexpr RrOp op(int k) { return k == DDPM3D_EM_MIN_Y ? RR_MIN : k == DDPM3D_EM_MAX_Y ? RR_MAX : RR_SUM; }
};

// Workgroup (part, b) reduces voxels [part * chunk, (part + 1) * chunk) of estimate b; chunk is a multiple of
// EM_THREADS * EM_VEC.  V = 4: 16-byte loads of x, y and std and one 4-byte load of the mask per thread and pass.
template <int V>
__global__ __launch_bounds__(EM_THREADS) void error_moments_kernel(
    const float* __restrict__ est, const float* __restrict__ target, const uint8_t* __restrict__ mask,
    const float* __restrict__ std, int64_t voxels, int64_t chunk, int parts, double* __restrict__ ws) {
    const int part = blockIdx.x, b = blockIdx.y;
    const int64_t v0 = (int64_t)part * chunk;
    const int64_t v1 = v0 + chunk < voxels ? v0 + chunk : voxels;
    const float* __restrict__ xb = est + (int64_t)b * voxels;
    double se = 0.0, sa = 0.0, sq = 0.0, sy = 0.0, syy = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    unsigned n = 0, c1 = 0, c2 = 0;       // at most chunk / EM_THREADS counts per thread
    for (int64_t i0 = v0 + (int64_t)threadIdx.x * V; i0 < v1; i0 += EM_THREADS * V) {
        float x[V], y[V], s[V];
        bool on[V];
        if constexpr (V == 4) {
            const float4 x4 = *reinterpret_cast<const float4*>(xb + i0);
            const float4 y4 = *reinterpret_cast<const float4*>(target + i0);
            x[0] = x4.x, x[1] = x4.y, x[2] = x4.z, x[3] = x4.w;
            y[0] = y4.x, y[1] = y4.y, y[2] = y4.z, y[3] = y4.w;
            unsigned m4 = 0x01010101u;
            if (mask) m4 = *reinterpret_cast<const unsigned*>(mask + i0);
#pragma unroll
            for (int v = 0; v < V; ++v) on[v] = ((m4 >> (8 * v)) & 0xffu) != 0;
            if (std) {
                const float4 s4 = *reinterpret_cast<const float4*>(std + i0);
                s[0] = s4.x, s[1] = s4.y, s[2] = s4.z, s[3] = s4.w;
            }
        } else {
            x[0] = xb[i0];
            y[0] = target[i0];
            on[0] = mask ? mask[i0] != 0 : true;
            if (std) s[0] = std[i0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (!on[v]) continue;
            const double yd = (double)y[v];
            const double e = (double)x[v] - yd;
            const double ae = fabs(e);
            n += 1;
            se += e;
            sa += ae;
            sq += e * e;
            sy += yd;
            syy += yd * yd;
            mn = fminf(mn, y[v]);
            mx = fmaxf(mx, y[v]);
            if (std) {
                const double sd = (double)s[v];
                c1 += ae <= sd;
                c2 += ae <= 2.0 * sd;
            }
        }
    }
    double rec[EM_REC];
    rec[DDPM3D_EM_N] = (double)n;
    rec[DDPM3D_EM_SUM_E] = se;
    rec[DDPM3D_EM_SUM_ABS_E] = sa;
    rec[DDPM3D_EM_SUM_SQ_E] = sq;
    rec[DDPM3D_EM_SUM_Y] = sy;
    rec[DDPM3D_EM_SUM_SQ_Y] = syy;
    rec[DDPM3D_EM_MIN_Y] = (double)mn;
    rec[DDPM3D_EM_MAX_Y] = (double)mx;
    rec[DDPM3D_EM_COVER_1] = (double)c1;
    rec[DDPM3D_EM_COVER_2] = (double)c2;
    rr_write_record<EmCols, EM_THREADS>(rec, ws + ((size_t)b * parts + part) * EM_REC);
}

// One workgroup per estimate: its records in a fixed order.
__global__ __launch_bounds__(EM_THREADS) void error_moments_fold_kernel(const double* __restrict__ ws, int parts,
                                                                        double* __restrict__ out) {
    const int b = blockIdx.x;
    rr_fold_record<EmCols, EM_THREADS>(ws + (size_t)b * parts * EM_REC, parts, out + (size_t)b * EM_REC);
}

// ---------------------------------------------------------------------------------------------- 3-D SSIM
// The march and the fold are ssim3d_body.h's, which the multi-scale entry (msssim.hip) shares.
__global__ __launch_bounds__(SS_THREADS) void ssim3d_kernel(
    const float* __restrict__ est, const float* __restrict__ target, const uint8_t* __restrict__ mask, int D, int H,
    int W, float C1, float C2, SsTaps taps, int chunk, int64_t recs, float* __restrict__ map,
    double* __restrict__ ws) {
    ssim3d_march<false>(est, target, mask, D, H, W, C1, C2, taps, chunk, recs, map, ws);
}

// One workgroup per estimate: {sum S, count} over its `used` records in a fixed order.
__global__ __launch_bounds__(256) void ssim3d_fold_kernel(const double* __restrict__ ws, int64_t recs, int used,
                                                          double* __restrict__ out) {
    ssim3d_fold<2>(ws, recs, used, out, 2);
}

}  // namespace

size_t ddpm3d_em_workspace_bytes(int B, int64_t voxels) {
    return rr_workspace_bytes(B, voxels, EM_THREADS * EM_VEC, EM_MAX_PARTS, EM_REC);
}

hipError_t ddpm3d_launch_error_moments(const float* est, const float* target, const uint8_t* mask, const float* std,
                                       int B, int64_t voxels, double* ws, double* out, hipStream_t st) {
    const RrPlan p = rr_plan(voxels, EM_THREADS * EM_VEC, EM_MAX_PARTS);
    const bool wide = voxels % EM_VEC == 0 && aligned(est, 16) && aligned(target, 16) && (!mask || aligned(mask, 4)) &&
                      (!std || aligned(std, 16));
    const dim3 grid(p.parts, B);
    if (wide)
        hipLaunchKernelGGL(error_moments_kernel<EM_VEC>, grid, dim3(EM_THREADS), 0, st, est, target, mask, std, voxels,
                           p.chunk, p.parts, ws);
    else
        hipLaunchKernelGGL(error_moments_kernel<1>, grid, dim3(EM_THREADS), 0, st, est, target, mask, std, voxels,
                           p.chunk, p.parts, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(error_moments_fold_kernel, dim3(B), dim3(EM_THREADS), 0, st, ws, p.parts, out);
    return hipGetLastError();
}

size_t ddpm3d_ss_workspace_bytes(int B, int D, int H, int W) {
    return (size_t)B * (size_t)ss_records(D, H, W) * 2 * sizeof(double);
}

hipError_t ddpm3d_launch_ssim3d(const float* est, const float* target, const uint8_t* mask, int B, int D, int H, int W,
                                float C1, float C2, double* ws, float* map, double* out, hipStream_t st) {
    const SsPlan p = ss_plan(D, H, W);
    const SsTaps taps = ss_taps();
    const int64_t recs = ss_records(D, H, W);
    const int tiles = p.tiles_w * p.tiles_h;
    hipLaunchKernelGGL(ssim3d_kernel, dim3(tiles, p.chunks, B), dim3(SS_THREADS), 0, st, est, target, mask, D, H, W,
                       C1, C2, taps, p.chunk, recs, map, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssim3d_fold_kernel, dim3(B), dim3(256), 0, st, ws, recs, tiles * p.chunks, out);
    return hipGetLastError();
}
