// Sliding-window tiling of a volume of any size: joint.hip's two kernels without a limit on the
// patches per axis.
//
// Layout as in joint.hip: canvas[b][z][x][y] (B draws of (Dc, H, W), W innermost), patch
// p = (ix * ny + iy) * nz + iz covers canvas[zs[iz] + 0..res)[xs[ix] + 0..res)[ys[iy] + 0..res), patch tensors are
// (patch, draw)-major: row p * B + b.  The starts live in device memory (ddpm3d_tiling.d_starts: xs, ys, zs back to
// back), not in the kernel arguments, so an axis may hold any number of them.
//
// tiles_blend_kernel is joint_blend_kernel's arithmetic, bit for bit: per voxel, over the covering patches in
// ascending p, acc = fl64(acc + fl64(fl64(x) * w)) with w = fl64(fl64(a_x * a_y) * a_z), one rounding to fp32.  The
// starts of an axis ascend (the C entries refuse anything else), so the patches that cover a coordinate are one run
// of indices; d_cover holds {first, count} of that run per coordinate and axis, and a voxel visits
// count_x * count_y * count_z patches (at most 8 where neighbours overlap by less than half a patch) instead of all
// nx * ny * nz.  Every index read from d_cover is clamped to the axis and every patch is still tested against the
// voxel, so a wrong table costs time or leaves a voxel short of a term; it cannot move a load outside the patches.
// One writer per element, no atomics, 64-bit offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int kMaxRowsPerLaunch = 65535;      // gridDim.z

// V consecutive elements along W per thread; V = 4 under joint.hip's rule (every y start, W and res a multiple of
// 4, both pointers 16-byte aligned).
template <int V>
__global__ __launch_bounds__(256) void tiles_gather_kernel(const float* __restrict__ canvas, int B, int Dc, int H,
                                                           int W, int res, int nx, int ny, int nz,
                                                           const int32_t* __restrict__ starts, int first_row,
                                                           float* __restrict__ out) {
    const int rq = res / V;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= res * rq) return;
    const int px = j / rq, py = (j - px * rq) * V, pz = blockIdx.y;
    const int row = first_row + blockIdx.z;                  // row of the whole (P * B) patch tensor
    const int p = row / B, b = row - p * B;
    const int ix = p / (ny * nz), iy = p / nz % ny, iz = p % nz;
    // clamped to the canvas: the entry has checked the host copy of the starts, this is the device copy
    const int x = min(max(starts[ix], 0), H - res) + px, y = min(max(starts[nx + iy], 0), W - res) + py,
              z = min(max(starts[nx + ny + iz], 0), Dc - res) + pz;
    float* o = out + (((int64_t)blockIdx.z * res + pz) * res + px) * res + py;
    const float* c = canvas + (((int64_t)b * Dc + z) * H + x) * W + y;
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(c);
    } else {
        *o = *c;
    }
}

template <int V>
__global__ __launch_bounds__(256) void tiles_blend_kernel(const float* __restrict__ patches, int B, int Dc, int H,
                                                          int W, int res, int nx, int ny, int nz,
                                                          const int32_t* __restrict__ starts,
                                                          const int32_t* __restrict__ cover,
                                                          const double* __restrict__ tables,
                                                          float* __restrict__ out) {
    // numpy rounds the product and the sum separately; hipcc would otherwise fuse them into one v_fma_f64
#pragma clang fp contract(off)
    const int wq = W / V;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= H * wq) return;
    const int x = j / wq, y0 = (j - x * wq) * V, z = blockIdx.y, b = blockIdx.z;
    const int32_t* xs = starts;
    const int32_t* ys = xs + nx;
    const int32_t* zs = ys + ny;
    const double* ax = tables;
    const double* ay = ax + (int64_t)nx * H;
    const double* az = ay + (int64_t)ny * W;
    const int2 cx = reinterpret_cast<const int2*>(cover)[x];
    const int2 cy = reinterpret_cast<const int2*>(cover)[H + y0];     // V = 4: the group is covered as a whole
    const int2 cz = reinterpret_cast<const int2*>(cover)[H + W + z];
    const int x0 = max(cx.x, 0), x1 = min(cx.x + cx.y, nx);
    const int yb = max(cy.x, 0), ye = min(cy.x + cy.y, ny);
    const int z0 = max(cz.x, 0), z1 = min(cz.x + cz.y, nz);
    const int64_t patch = (int64_t)res * res * res;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
    for (int ix = x0; ix < x1; ++ix) {
        const int px = x - xs[ix];
        if (px < 0 || px >= res) continue;
        const double wx = ax[(int64_t)ix * H + x];
        for (int iy = yb; iy < ye; ++iy) {
            const int py = y0 - ys[iy];
            if (py < 0 || py > res - V) continue;
            double wxy[V];
#pragma unroll
            for (int v = 0; v < V; ++v) wxy[v] = wx * ay[(int64_t)iy * W + y0 + v];
            for (int iz = z0; iz < z1; ++iz) {
                const int pz = z - zs[iz];
                if (pz < 0 || pz >= res) continue;
                const double wz = az[(int64_t)iz * Dc + z];
                const int64_t row = ((int64_t)(ix * ny + iy) * nz + iz) * B + b;
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

// every y start, W and res a multiple of 4: the four-wide forms apply (joint.hip's quads())
bool quads(const ddpm3d_tiling& t, int W, int res) {
    if (W % 4 || res % 4) return false;
    for (int i = 0; i < t.n[1]; ++i)
        if (t.starts[1][i] % 4) return false;
    return true;
}

}  // namespace

hipError_t ddpm3d_launch_tiles_gather(const float* canvas, int B, int Dc, int H, int W, int res,
                                      const ddpm3d_tiling& t, int first_patch, int n_patches, float* out,
                                      hipStream_t st) {
    const bool v4 = quads(t, W, res) && aligned16(canvas) && aligned16(out);
    const int per_plane = res * (res / (v4 ? 4 : 1));
    const int64_t rows = (int64_t)n_patches * B, patch = (int64_t)res * res * res;
    // the rows ride on gridDim.z: at most 65535 per launch
    for (int64_t r0 = 0; r0 < rows; r0 += kMaxRowsPerLaunch) {
        const int n = (int)(rows - r0 < kMaxRowsPerLaunch ? rows - r0 : kMaxRowsPerLaunch);
        const dim3 grid((per_plane + 255) / 256, res, n);
        const int first_row = (int)((int64_t)first_patch * B + r0);
        float* o = out + r0 * patch;
        if (v4)
            hipLaunchKernelGGL(tiles_gather_kernel<4>, grid, dim3(256), 0, st, canvas, B, Dc, H, W, res, t.n[0],
                               t.n[1], t.n[2], t.d_starts, first_row, o);
        else
            hipLaunchKernelGGL(tiles_gather_kernel<1>, grid, dim3(256), 0, st, canvas, B, Dc, H, W, res, t.n[0],
                               t.n[1], t.n[2], t.d_starts, first_row, o);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t ddpm3d_launch_tiles_blend(const float* patches, int B, int Dc, int H, int W, int res,
                                     const ddpm3d_tiling& t, float* out, hipStream_t st) {
    const bool v4 = quads(t, W, res) && aligned16(patches) && aligned16(out);
    const int per_plane = H * (W / (v4 ? 4 : 1));
    const dim3 grid((per_plane + 255) / 256, Dc, B);
    if (v4)
        hipLaunchKernelGGL(tiles_blend_kernel<4>, grid, dim3(256), 0, st, patches, B, Dc, H, W, res, t.n[0], t.n[1],
                           t.n[2], t.d_starts, t.d_cover, t.d_tables, out);
    else
        hipLaunchKernelGGL(tiles_blend_kernel<1>, grid, dim3(256), 0, st, patches, B, Dc, H, W, res, t.n[0], t.n[1],
                           t.n[2], t.d_starts, t.d_cover, t.d_tables, out);
    return hipGetLastError();
}
