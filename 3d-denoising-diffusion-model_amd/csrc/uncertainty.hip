// Per-voxel uncertainty maps from K posterior draws of one volume.
//
// draw_stitch_kernel adds one patch origin's K draws into K full-volume accumulators with the reference's Hann
// blend (scripts/test.py:141-142), bit for bit as numpy evaluates it: acc = fl32(fl64(acc) + fl64(x) * w) with the
// fp64 window w, and wsum = fl32(fl64(wsum) + w).  draw_moments_kernel divides every accumulator by the weight
// (scripts/test.py:146, a correctly rounded fp32 division as np.divide does) and reduces the K volumes to mean
// and sample std (ddof = 1) in fp64 registers.  Both kernels are HBM-bound; offsets are 64-bit (K * voxels of a
// whole-body volume passes 2^31 elements) and each output element has exactly one writer: no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ops.h"

namespace {

constexpr int ST_TILE = 32;            // a 32 (W) x 32 (Z) tile of one H row of the patch per workgroup
constexpr int ST_ROWS = 8;             // 256 threads = 32 x 8, four tile rows per thread

// The patch comes as the sampler writes it, x[d][z][h][w] (NCDHW, C = 1, W innermost); the volume is
// acc[d][X][Y][Z] (the reference's (H, W, Z) layout, Z innermost).  The tile goes through LDS so that both the
// read (along w) and the read-modify-write (along z) are contiguous.
__global__ __launch_bounds__(ST_TILE * ST_ROWS) void draw_stitch_kernel(
    const float* __restrict__ x, int K, int res, const double* __restrict__ win, int xs, int ys, int zs, int H,
    int W, int D, int wy, int dz, float* __restrict__ acc, float* __restrict__ wsum) {
    // numpy rounds the product and the sum separately; hipcc would otherwise fuse them into one v_fma_f64 (the
    // __dmul_rn / __dadd_rn wrappers are plain operators and get contracted too)
#pragma clang fp contract(off)
    __shared__ float tile[ST_TILE][ST_TILE + 1];
    const int tx = threadIdx.x % ST_TILE, ty = threadIdx.x / ST_TILE;
    const int w0 = blockIdx.x * ST_TILE, z0 = blockIdx.y * ST_TILE, h = blockIdx.z;
    const int64_t patch = (int64_t)res * res * res;
    const int64_t vol = (int64_t)H * W * D;

    // this thread's four output points: (w = w0 + r, z = z0 + tx) for r = ty, ty + 8, ...
    double wv[ST_TILE / ST_ROWS];
    int64_t off[ST_TILE / ST_ROWS];
    bool in[ST_TILE / ST_ROWS];
#pragma unroll
    for (int i = 0; i < ST_TILE / ST_ROWS; ++i) {
        const int w = w0 + ty + i * ST_ROWS, z = z0 + tx;
        in[i] = w < wy && z < dz;
        wv[i] = in[i] ? win[((int64_t)h * res + w) * res + z] : 0.0;
        off[i] = ((int64_t)(xs + h) * W + (ys + w)) * D + (zs + z);
        if (in[i]) wsum[off[i]] = (float)((double)wsum[off[i]] + wv[i]);
    }
    for (int d = 0; d < K; ++d) {
        const float* xd = x + d * patch;
#pragma unroll
        for (int i = 0; i < ST_TILE / ST_ROWS; ++i) {
            const int z = z0 + ty + i * ST_ROWS, w = w0 + tx;
            if (z < dz && w < wy) tile[ty + i * ST_ROWS][tx] = xd[((int64_t)z * res + h) * res + w];
        }
        __syncthreads();
        float* ad = acc + d * vol;
#pragma unroll
        for (int i = 0; i < ST_TILE / ST_ROWS; ++i) {
            if (!in[i]) continue;
            const double prod = (double)tile[tx][ty + i * ST_ROWS] * wv[i];
            ad[off[i]] = (float)((double)ad[off[i]] + prod);
        }
        __syncthreads();
    }
}

// V consecutive voxels per thread (V = 4: float4 loads when voxels % 4 == 0 and every pointer is 16-byte aligned).
// Welford's update in fp64: no cancellation when the draws' spread is tiny beside their mean.
template <int V>
__global__ __launch_bounds__(256) void draw_moments_kernel(const float* __restrict__ acc,
                                                           const float* __restrict__ wsum, int K, int64_t voxels,
                                                           float* __restrict__ mean, float* __restrict__ std) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i0 >= voxels) return;
    float ws[V];
    bool live[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        ws[v] = 1.0f;
        live[v] = i0 + v < voxels;
    }
    if (wsum) {
        if constexpr (V == 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(wsum + i0);
            ws[0] = w4.x, ws[1] = w4.y, ws[2] = w4.z, ws[3] = w4.w;
        } else {
            ws[0] = wsum[i0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) live[v] = live[v] && ws[v] > 0.0f;
    }
    double m[V], m2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) m[v] = m2[v] = 0.0;
#pragma unroll 4
    for (int d = 0; d < K; ++d) {
        float a[V];
        if constexpr (V == 4) {
            const float4 a4 = *reinterpret_cast<const float4*>(acc + d * voxels + i0);
            a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
        } else {
            a[0] = acc[d * voxels + i0];
        }
        const double inv = 1.0 / (double)(d + 1);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const double xv = wsum && live[v] ? (double)__fdiv_rn(a[v], ws[v]) : (double)a[v];
            const double delta = xv - m[v];
            m[v] += delta * inv;
            m2[v] += delta * (xv - m[v]);
        }
    }
    float mo[V], so[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        mo[v] = live[v] ? (float)m[v] : 0.0f;
        so[v] = live[v] ? (float)sqrt(fmax(m2[v], 0.0) / (double)(K - 1)) : 0.0f;
    }
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(mean + i0) = make_float4(mo[0], mo[1], mo[2], mo[3]);
        *reinterpret_cast<float4*>(std + i0) = make_float4(so[0], so[1], so[2], so[3]);
    } else {
        mean[i0] = mo[0];
        std[i0] = so[0];
    }
}

}  // namespace

hipError_t ddpm3d_launch_draw_stitch(const float* samples, int K, int res, const double* window, int xs, int ys,
                                     int zs, int H, int W, int D, float* acc, float* wsum, hipStream_t st) {
    const int hx = H - xs < res ? H - xs : res, wy = W - ys < res ? W - ys : res, dz = D - zs < res ? D - zs : res;
    const dim3 grid((wy + ST_TILE - 1) / ST_TILE, (dz + ST_TILE - 1) / ST_TILE, hx);
    hipLaunchKernelGGL(draw_stitch_kernel, grid, dim3(ST_TILE * ST_ROWS), 0, st, samples, K, res, window, xs, ys, zs,
                       H, W, D, wy, dz, acc, wsum);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_draw_moments(const float* acc, const float* wsum, int K, int64_t voxels, float* mean,
                                      float* std, hipStream_t st) {
    if (voxels % 4 == 0 && aligned16(acc) && (!wsum || aligned16(wsum)) && aligned16(mean) && aligned16(std)) {
        const int64_t blocks = (voxels / 4 + 255) / 256;
        hipLaunchKernelGGL(draw_moments_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, acc, wsum, K, voxels,
                           mean, std);
    } else {
        const int64_t blocks = (voxels + 255) / 256;
        hipLaunchKernelGGL(draw_moments_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, acc, wsum, K, voxels,
                           mean, std);
    }
    return hipGetLastError();
}
