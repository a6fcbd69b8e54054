// Joint patch sampling: one state per volume, cut into overlapping patches before every network
// call and blended back after every reverse step.
//
// The canvas is canvas[b][z][x][y] (B draws, (Dc, H, W), W innermost: the patches' own (Z, H, W) order); patch
// p = (ix * ny + iy) * nz + iz covers canvas[zs[iz] + 0..res)[xs[ix] + 0..res)[ys[iy] + 0..res), and the patch
// tensors are (patch, draw)-major: row p * B + b.
//
// Every patch lies inside the canvas (0 <= start <= extent - res on each axis; the C entries refuse anything else), so
// joint_gather_kernel is a plain copy, canvas -> patches.  joint_blend_kernel is the normalised Hann blend in gather
// form: one thread per canvas voxel (or per four along W) walks the covering (ix, iy, iz) in ascending p and
// evaluates patches.joint_blend bit for bit, acc = fl64(acc + fl64(fl64(x) * w)) with w = fl64(fl64(a_x * a_y) * a_z),
// one rounding to fp32 at the end.  One writer per element, no atomics, 64-bit offsets.  Both kernels are HBM-bound;
// the per-axis tables (a few KB) stay in cache.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

// V consecutive elements along W per thread.  V = 4 needs every y start, W and res to be multiples of 4 (a group
// of four is then inside or outside a patch as a whole, and 16-byte aligned on both sides).
template <int V>
__global__ __launch_bounds__(256) void joint_gather_kernel(const float* __restrict__ canvas, int B, int Dc, int H,
                                                           int W, int res, ddpm3d_joint_starts s, int first_patch,
                                                           float* __restrict__ out) {
    const int rq = res / V;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= res * rq) return;
    const int px = j / rq, py = (j - px * rq) * V, pz = blockIdx.y;
    const int row = blockIdx.z, p = first_patch + row / B, b = row % B;
    const int ix = p / (s.ny * s.nz), iy = p / s.nz % s.ny, iz = p % s.nz;
    const int x = s.xs[ix] + px, y = s.ys[iy] + py, z = s.zs[iz] + pz;
    float* o = out + (((int64_t)row * res + pz) * res + px) * res + py;
    const float* c = canvas + (((int64_t)b * Dc + z) * H + x) * W + y;
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(c);
    } else {
        *o = *c;
    }
}

template <int V>
__global__ __launch_bounds__(256) void joint_blend_kernel(const float* __restrict__ patches, int B, int Dc, int H,
                                                          int W, int res, ddpm3d_joint_starts s,
                                                          const double* __restrict__ tables,
                                                          float* __restrict__ out) {
    // numpy rounds the product and the sum separately; hipcc would otherwise fuse them into one v_fma_f64
#pragma clang fp contract(off)
    const int wq = W / V;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= H * wq) return;
    const int x = j / wq, y0 = (j - x * wq) * V, z = blockIdx.y, b = blockIdx.z;
    const double* ax = tables;
    const double* ay = ax + (int64_t)s.nx * H;
    const double* az = ay + (int64_t)s.ny * W;
    const int64_t patch = (int64_t)res * res * res;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
    for (int ix = 0; ix < s.nx; ++ix) {
        const int px = x - s.xs[ix];
        if (px < 0 || px >= res) continue;
        const double wx = ax[(int64_t)ix * H + x];
        for (int iy = 0; iy < s.ny; ++iy) {
            const int py = y0 - s.ys[iy];
            // V = 4: the group is covered as a whole; V = 1: this element
            if (py < 0 || py >= res) continue;
            double wxy[V];
#pragma unroll
            for (int v = 0; v < V; ++v) wxy[v] = wx * ay[(int64_t)iy * W + y0 + v];
            for (int iz = 0; iz < s.nz; ++iz) {
                const int pz = z - s.zs[iz];
                if (pz < 0 || pz >= res) continue;
                const double wz = az[(int64_t)iz * Dc + z];
                const int64_t row = (int64_t)((ix * s.ny + iy) * s.nz + iz) * B + b;
                const float* src = patches + row * patch + ((int64_t)pz * res + px) * res + py;
                float xv[V];
                if constexpr (V == 4) {
                    const float4 x4 = *reinterpret_cast<const float4*>(src);
                    xv[0] = x4.x, xv[1] = x4.y, xv[2] = x4.z, xv[3] = x4.w;
                } else {
                    xv[0] = *src;
                }
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double w = wxy[v] * wz;
                    const double prod = (double)xv[v] * w;
                    acc[v] = acc[v] + prod;
                }
            }
        }
    }
    float* o = out + (((int64_t)b * Dc + z) * H + x) * W + y0;
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(o) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    } else {
        *o = (float)acc[0];
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// every y start, W and res a multiple of 4: the four-wide forms apply
bool quads(const ddpm3d_joint_starts& s, int W, int res) {
    if (W % 4 || res % 4) return false;
    for (int i = 0; i < s.ny; ++i)
        if (s.ys[i] % 4) return false;
    return true;
}

}  // namespace

hipError_t ddpm3d_launch_joint_gather(const float* canvas, int B, int Dc, int H, int W, int res,
                                      const ddpm3d_joint_starts& s, int first_patch, int n_patches, float* out,
                                      hipStream_t st) {
    const bool v4 = quads(s, W, res) && aligned16(canvas) && aligned16(out);
    const int per_plane = res * (res / (v4 ? 4 : 1));
    const dim3 grid((per_plane + 255) / 256, res, n_patches * B);
    if (v4)
        hipLaunchKernelGGL(joint_gather_kernel<4>, grid, dim3(256), 0, st, canvas, B, Dc, H, W, res, s, first_patch,
                           out);
    else
        hipLaunchKernelGGL(joint_gather_kernel<1>, grid, dim3(256), 0, st, canvas, B, Dc, H, W, res, s, first_patch,
                           out);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_joint_blend(const float* patches, int B, int Dc, int H, int W, int res,
                                     const ddpm3d_joint_starts& s, const double* tables, float* out, hipStream_t st) {
    const bool v4 = quads(s, W, res) && aligned16(patches) && aligned16(out);
    const int per_plane = H * (W / (v4 ? 4 : 1));
    const dim3 grid((per_plane + 255) / 256, Dc, B);
    if (v4)
        hipLaunchKernelGGL(joint_blend_kernel<4>, grid, dim3(256), 0, st, patches, B, Dc, H, W, res, s, tables, out);
    else
        hipLaunchKernelGGL(joint_blend_kernel<1>, grid, dim3(256), 0, st, patches, B, Dc, H, W, res, s, tables, out);
    return hipGetLastError();
}
