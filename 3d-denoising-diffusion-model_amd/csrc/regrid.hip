// Volume regridding between two voxel grids (definitions in include/ddpm3d.h): one banded linear map
// per axis, applied as one launch per non-identity axis in the order W, H, D.  The passes chain vol -> ... -> out
// through the caller's workspace, so that vol is only read and the last pass writes out; with no pass at all out is a
// device-to-device copy of vol.  A pass sees its input as [outer][Li][inner] and writes [outer][Lo][inner]: inner is 1
// along W, the current row length along H and the current plane along D.  An output voxel adds its counted taps in
// ascending input index, the first as a product and the others by fma (one rounding per tap); the weights are
// normalised on the host, so nothing is divided.  No atomics; volume b is a grid coordinate and sees nothing of the
// others.  Two kernels of the same arithmetic:
//   regrid_row_kernel   H and D passes whose inner is a multiple of 4, at least ROW_MIN_INNER and 16-byte aligned: a
//                       wave owns 256 consecutive words of one output row, so the output index, first, count and the
//                       weights are wave-uniform, a lane moves 16 bytes per tap and there is no integer division
//   regrid_voxel_kernel everything else (the W pass among it): a thread owns a few output voxels; lanes read first,
//                       count and weights[tap][o] at consecutive o
// Both load every tap before the first multiply (the tap capacity is a template argument, the loops are unrolled), so
// that the loads of a voxel are in flight together.
// The tables are device memory the host cannot check: count is clamped to the axis's tap capacity and every input
// index to [0, Li - 1] here, so that a bad table gives wrong numbers and never a read outside vol.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int REGRID_THREADS = 256;
constexpr int ROW_WAVES = 4;                                  // waves (output rows) per workgroup of the row kernel
constexpr int ROW_CHUNK = 256;                                // words of a row per wave: 64 lanes x float4
constexpr int64_t ROW_MIN_INNER = 128;
constexpr int64_t ROW_MAX_INNER = (int64_t)65535 * ROW_CHUNK; // gridDim.y

struct RegridPass {
    int64_t in_voxels, out_voxels;                            // per volume, before and after this pass
    uint32_t inner;                                           // words between neighbours along the pass's axis
    uint32_t rows;                                            // outer * Lo: output rows of `inner` words
    int Li, Lo, taps;
};

__device__ __forceinline__ int clamp_count(int n, int taps) { return n < 0 ? 0 : n > taps ? taps : n; }
__device__ __forceinline__ int clamp_index(int k, int L) { return k < 0 ? 0 : k > L - 1 ? L - 1 : k; }

// ITEMS output voxels per thread, a whole grid apart (every load and store of a wave stays contiguous in o): the loads
// of all of them are issued before the first multiply.  The loads do not depend on count[o] -- a tap at or beyond it
// is read at a clamped index inside the volume and dropped by a select, never multiplied, so that it cannot carry a
// NaN into the sum -- because a load under a per-lane condition waits for the one before it.
template <int CAP, int ITEMS>
__global__ __launch_bounds__(REGRID_THREADS) void regrid_voxel_kernel(const float* __restrict__ in,
                                                                      float* __restrict__ out,
                                                                      const int32_t* __restrict__ first,
                                                                      const int32_t* __restrict__ count,
                                                                      const float* __restrict__ weights,
                                                                      const RegridPass p) {
    const int64_t t0 = (int64_t)blockIdx.x * REGRID_THREADS + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * REGRID_THREADS;
    const float* vol = in + (int64_t)blockIdx.y * p.in_voxels;
    const int cap = p.taps < CAP ? p.taps : CAP;              // the table holds `taps` rows of weights
    uint32_t o[ITEMS];
    const float* src[ITEMS];
    int n[ITEMS], f[ITEMS];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i64 = t0 + j * step;
        // out_voxels <= 2^31 - 1 (the host has checked); an item past the end works on the last voxel and stores nothing
        const uint32_t i = (uint32_t)(i64 < p.out_voxels ? i64 : p.out_voxels - 1);
        const uint32_t q = i / p.inner, x = i - q * p.inner;
        const uint32_t outer = q / (uint32_t)p.Lo;
        o[j] = q - outer * (uint32_t)p.Lo;
        src[j] = vol + (int64_t)outer * p.Li * p.inner + x;
        n[j] = count[o[j]], f[j] = first[o[j]];
    }
    float v[ITEMS][CAP], w[ITEMS][CAP];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        n[j] = clamp_count(n[j], cap), f[j] = clamp_index(f[j], p.Li);
#pragma unroll
        for (int t = 0; t < CAP; ++t)
            if (t < cap) {                                    // the same for every lane
                v[j][t] = src[j][(int64_t)clamp_index(f[j] + t, p.Li) * p.inner];
                w[j][t] = weights[(int64_t)t * p.Lo + o[j]];
            }
    }
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int t = 0; t < CAP; ++t)
            if (t < cap) {
                const float next = t == 0 ? w[j][0] * v[j][0] : __builtin_fmaf(w[j][t], v[j][t], acc);
                acc = t < n[j] ? next : acc;                  // only counted taps enter the sum
            }
        const int64_t i64 = t0 + j * step;
        if (i64 < p.out_voxels) out[(int64_t)blockIdx.y * p.out_voxels + i64] = acc;
    }
}

template <int CAP>
__global__ __launch_bounds__(64 * ROW_WAVES) void regrid_row_kernel(const float* __restrict__ in,
                                                                    float* __restrict__ out,
                                                                    const int32_t* __restrict__ first,
                                                                    const int32_t* __restrict__ count,
                                                                    const float* __restrict__ weights,
                                                                    const RegridPass p) {
    // the output row of this wave: the same for its 64 lanes
    const uint32_t q = __builtin_amdgcn_readfirstlane(blockIdx.x * ROW_WAVES + threadIdx.y);
    const uint32_t x = (blockIdx.y * 64 + threadIdx.x) * 4;
    if (q >= p.rows || x >= p.inner) return;                  // inner is a multiple of 4: a lane's 4 words lie in the row
    const uint32_t outer = q / (uint32_t)p.Lo, o = q - outer * (uint32_t)p.Lo;
    const int n = clamp_count(count[o], p.taps < CAP ? p.taps : CAP);
    const int f = clamp_index(first[o], p.Li);
    const float* src = in + (int64_t)blockIdx.z * p.in_voxels + (int64_t)outer * p.Li * p.inner + x;
    float4 v[CAP];
    float w[CAP];
#pragma unroll
    for (int t = 0; t < CAP; ++t)                             // taps at or beyond count[o] are never read
        if (t < n) {
            v[t] = *reinterpret_cast<const float4*>(src + (int64_t)clamp_index(f + t, p.Li) * p.inner);
            w[t] = weights[(int64_t)t * p.Lo + o];
        }
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int t = 0; t < CAP; ++t)
        if (t < n) {
            if (t == 0) {
                acc = make_float4(w[0] * v[0].x, w[0] * v[0].y, w[0] * v[0].z, w[0] * v[0].w);
            } else {
                acc.x = __builtin_fmaf(w[t], v[t].x, acc.x);
                acc.y = __builtin_fmaf(w[t], v[t].y, acc.y);
                acc.z = __builtin_fmaf(w[t], v[t].z, acc.z);
                acc.w = __builtin_fmaf(w[t], v[t].w, acc.w);
            }
        }
    *reinterpret_cast<float4*>(out + (int64_t)blockIdx.z * p.out_voxels + (int64_t)q * p.inner + x) = acc;
}

template <int CAP>
hipError_t launch_pass(const float* src, float* dst, const ddpm3d_regrid_axis& a, const RegridPass& p, int B,
                       hipStream_t st) {
    // rows of a volume start at multiples of inner words, volumes at multiples of in_voxels / out_voxels: with inner a
    // multiple of 4 both are multiples of 4 words, so 16-byte aligned buffers make every float4 aligned
    const bool row = p.inner % 4 == 0 && p.inner >= ROW_MIN_INNER && p.inner <= ROW_MAX_INNER && aligned16(src) &&
                     aligned16(dst);
    if (row) {
        const dim3 grid((p.rows + ROW_WAVES - 1) / ROW_WAVES, (p.inner + ROW_CHUNK - 1) / ROW_CHUNK, (unsigned)B);
        hipLaunchKernelGGL(regrid_row_kernel<CAP>, grid, dim3(64, ROW_WAVES), 0, st, src, dst, a.first, a.count,
                           a.weights, p);
    } else {
        constexpr int ITEMS = CAP <= 8 ? 4 : 2;
        const int64_t per_block = (int64_t)REGRID_THREADS * ITEMS;
        const unsigned blocks = (unsigned)((p.out_voxels + per_block - 1) / per_block);             // at most 2^22
        hipLaunchKernelGGL((regrid_voxel_kernel<CAP, ITEMS>), dim3(blocks, (unsigned)B), dim3(REGRID_THREADS), 0, st,
                           src, dst, a.first, a.count, a.weights, p);
    }
    return hipGetLastError();
}

}  // namespace

void ddpm3d_regrid_stages(int D, int H, int W, int Do, int Ho, int Wo, int64_t stage[3]) {
    stage[0] = (int64_t)D * H * Wo;
    stage[1] = (int64_t)D * Ho * Wo;
    stage[2] = (int64_t)Do * Ho * Wo;
}

hipError_t ddpm3d_launch_regrid(const float* vol, int B, int D, int H, int W, const ddpm3d_regrid_axis* axes,
                                float* out, float* ws, hipStream_t st) {
    const ddpm3d_regrid_axis& aD = axes[0];
    const ddpm3d_regrid_axis& aH = axes[1];
    const ddpm3d_regrid_axis& aW = axes[2];
    const int Do = aD.out_len, Ho = aH.out_len, Wo = aW.out_len;
    int64_t stage[3];
    ddpm3d_regrid_stages(D, H, W, Do, Ho, Wo, stage);
    const int64_t in_voxels = (int64_t)D * H * W;
    // pass order W, H, D; the input of each pass has the extents its predecessors left
    const ddpm3d_regrid_axis* axis[3] = {&aW, &aH, &aD};
    const int64_t inner[3] = {1, Wo, (int64_t)Ho * Wo};
    const int64_t before[3] = {in_voxels, stage[0], stage[1]};
    int passes = 0;
    for (int k = 0; k < 3; ++k) passes += axis[k]->taps > 0;
    if (passes == 0)
        return hipMemcpyAsync(out, vol, (size_t)B * in_voxels * sizeof(float), hipMemcpyDeviceToDevice, st);
    // the two intermediate buffers of the workspace: the W pass's output, then the H pass's
    float* buf[2] = {ws, ws + (((size_t)B * stage[0] + 3) & ~(size_t)3)};
    const float* src = vol;
    int done = 0;
    for (int k = 0; k < 3; ++k) {
        const ddpm3d_regrid_axis& a = *axis[k];
        if (a.taps == 0) continue;
        ++done;
        float* dst = done == passes ? out : buf[k];
        RegridPass p;
        p.in_voxels = before[k], p.out_voxels = stage[k], p.inner = (uint32_t)inner[k];
        p.rows = (uint32_t)(stage[k] / inner[k]);
        p.Li = a.in_len, p.Lo = a.out_len, p.taps = a.taps;
        const hipError_t e = a.taps <= 2   ? launch_pass<2>(src, dst, a, p, B, st)
                             : a.taps <= 4 ? launch_pass<4>(src, dst, a, p, B, st)
                             : a.taps <= 8 ? launch_pass<8>(src, dst, a, p, B, st)
                                           : launch_pass<DDPM3D_REGRID_MAX_TAPS>(src, dst, a, p, B, st);
        if (e != hipSuccess) return e;
        src = dst;
    }
    return hipSuccess;
}
