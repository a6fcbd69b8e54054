// Cutting B canvases into overlapping patches and blending updated patches back: the two kernels of joint patch
// sampling and of the sliding-window tiling of a volume of any size.
//
// The canvas is canvas[b][z][x][y] (B draws of (Dc, H, W), W innermost: the patches' own (Z, H, W) order); patch
// p = (ix * ny + iy) * nz + iz covers canvas[zs[iz] + 0..res)[xs[ix] + 0..res)[ys[iy] + 0..res), and the patch
// tensors are (patch, draw)-major: row p * B + b.  Every patch lies inside the canvas (0 <= start <= extent - res on
// each axis; the C entries refuse anything else), so patch_gather_kernel is a plain copy, canvas -> patches.
// patch_blend_kernel is the normalised Hann blend in gather form: one thread per canvas voxel (or per four along W)
// walks covering (ix, iy, iz) in ascending p and evaluates patches.joint_blend bit for bit,
// acc = fl64(acc + fl64(fl64(x) * w)) with w = fl64(fl64(a_x * a_y) * a_z), one rounding to fp32 at the end.  One
// writer per element, no atomics, 64-bit offsets.  Both kernels are HBM-bound; the per-axis tables (a few KB) stay
// in cache.
//
// Each kernel is one body, instantiated per width and per `Starts` policy; the policies differ in where a start comes
// from and in which patch indices a voxel walks, and in nothing else:
//   StartsByValue   (ddpm3d_joint_*): a ddpm3d_joint_starts in the kernel arguments, at most DDPM3D_JOINT_MAX_STARTS
//       per axis, in any order and with repeats; a voxel walks all nx * ny * nz patches.
//   StartsInMemory  (ddpm3d_tiles_*): ddpm3d_tiling.d_starts (xs, ys, zs back to back), any number per axis.  The
//       starts of an axis ascend (the C entries refuse anything else), so the patches that cover a coordinate are one
//       run of indices; d_cover holds {first, count} of that run per coordinate and axis, and a voxel visits
//       count_x * count_y * count_z patches (at most 8 where neighbours overlap by less than half a patch).  Every
//       index read from d_cover is clamped to the axis and every patch is still tested against the voxel, so a wrong
//       table costs time or leaves a voxel short of a term; it cannot move a load outside the patches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int kMaxRowsPerLaunch = 65535;      // gridDim.z

// Axes are 0, 1, 2 = H, W, D.  n(a): the patches on the axis; start(a, i): the start of patch i; placed(a, i, last):
// the same as the gather uses it, inside [0, last]; run(a, k): the patch indices {first, end} to walk for a
// coordinate, k being the coordinate's place in the H, then W, then Dc coordinates back to back.
struct StartsByValue {
    ddpm3d_joint_starts s;
    __device__ int n(int a) const { return a == 0 ? s.nx : a == 1 ? s.ny : s.nz; }
    __device__ int start(int a, int i) const { return (a == 0 ? s.xs : a == 1 ? s.ys : s.zs)[i]; }
    // the host copy is the only copy and the entry has checked it: no clamp
    __device__ int placed(int a, int i, int) const { return start(a, i); }
    __device__ int2 run(int a, int) const { return make_int2(0, n(a)); }
};

struct StartsInMemory {
    int nx, ny, nz;
    const int32_t* d_starts;
    const int32_t* d_cover;
    __device__ int n(int a) const { return a == 0 ? nx : a == 1 ? ny : nz; }
    __device__ int start(int a, int i) const { return d_starts[(a == 0 ? 0 : a == 1 ? nx : nx + ny) + i]; }
    // the entry has checked the host copy of the starts, this is the device copy
    __device__ int placed(int a, int i, int last) const { return min(max(start(a, i), 0), last); }
    __device__ int2 run(int a, int k) const {
        const int2 c = reinterpret_cast<const int2*>(d_cover)[k];
        return make_int2(max(c.x, 0), min(c.x + c.y, n(a)));
    }
};

// V consecutive elements along W per thread.  V = 4 needs every y start, W and res to be multiples of 4 (a group
// of four is then inside or outside a patch as a whole, and 16-byte aligned on both sides); see quads().
// Writes rows [first_row, first_row + gridDim.z) of the whole (P * B) patch tensor to out[gridDim.z][res^3].
template <int V, class Starts>
__global__ __launch_bounds__(256) void patch_gather_kernel(const float* __restrict__ canvas, int B, int Dc, int H,
                                                           int W, int res, Starts s, int first_row,
                                                           float* __restrict__ out) {
    const int rq = res / V;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= res * rq) return;
    const int px = j / rq, py = (j - px * rq) * V, pz = blockIdx.y;
    const int row = first_row + blockIdx.z;
    const int p = row / B, b = row - p * B;
    const int ny = s.n(1), nz = s.n(2);
    const int ix = p / (ny * nz), iy = p / nz % ny, iz = p % nz;
    const int x = s.placed(0, ix, H - res) + px, y = s.placed(1, iy, W - res) + py,
              z = s.placed(2, iz, Dc - res) + pz;
    float* o = out + (((int64_t)blockIdx.z * res + pz) * res + px) * res + py;
    const float* c = canvas + (((int64_t)b * Dc + z) * H + x) * W + y;
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(c);
    } else {
        *o = *c;
    }
}

template <int V, class Starts>
__global__ __launch_bounds__(256) void patch_blend_kernel(const float* __restrict__ patches, int B, int Dc, int H,
                                                          int W, int res, Starts s,
                                                          const double* __restrict__ tables,
                                                          float* __restrict__ out) {
    // numpy rounds the product and the sum separately; hipcc would otherwise fuse them into one v_fma_f64
#pragma clang fp contract(off)
    const int wq = W / V;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= H * wq) return;
    const int x = j / wq, y0 = (j - x * wq) * V, z = blockIdx.y, b = blockIdx.z;
    const int nx = s.n(0), ny = s.n(1), nz = s.n(2);
    const double* ax = tables;
    const double* ay = ax + (int64_t)nx * H;
    const double* az = ay + (int64_t)ny * W;
    const int2 rx = s.run(0, x), ry = s.run(1, H + y0), rz = s.run(2, H + W + z);
    const int64_t patch = (int64_t)res * res * res;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
    for (int ix = rx.x; ix < rx.y; ++ix) {
        const int px = x - s.start(0, ix);
        if (px < 0 || px >= res) continue;
        const double wx = ax[(int64_t)ix * H + x];
        for (int iy = ry.x; iy < ry.y; ++iy) {
            const int py = y0 - s.start(1, iy);
            // all V elements inside the patch.  V = 4 runs under quads(): y0, the start and res are multiples of 4,
            // so is py, and py > res - 4 is py >= res: the group is covered as a whole or not at all
            if (py < 0 || py > res - V) continue;
            double wxy[V];
#pragma unroll
            for (int v = 0; v < V; ++v) wxy[v] = wx * ay[(int64_t)iy * W + y0 + v];
            for (int iz = rz.x; iz < rz.y; ++iz) {
                const int pz = z - s.start(2, iz);
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

// every y start (host copy), W and res a multiple of 4: the four-wide forms apply
bool quads(int ny, const int32_t* ys, int W, int res) {
    if (W % 4 || res % 4) return false;
    for (int i = 0; i < ny; ++i)
        if (ys[i] % 4) return false;
    return true;
}

// rows [first_row, first_row + rows) of the patch tensor -> out; the rows ride on gridDim.z, at most 65535 per launch
template <class Starts>
hipError_t launch_gather(const float* canvas, int B, int Dc, int H, int W, int res, const Starts& s, bool v4,
                         int64_t first_row, int64_t rows, float* out, hipStream_t st) {
    const int per_plane = res * (res / (v4 ? 4 : 1));
    const int64_t patch = (int64_t)res * res * res;
    for (int64_t r0 = 0; r0 < rows; r0 += kMaxRowsPerLaunch) {
        const int n = (int)(rows - r0 < kMaxRowsPerLaunch ? rows - r0 : kMaxRowsPerLaunch);
        const dim3 grid((per_plane + 255) / 256, res, n);
        const auto kernel = v4 ? patch_gather_kernel<4, Starts> : patch_gather_kernel<1, Starts>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, canvas, B, Dc, H, W, res, s, (int)(first_row + r0),
                           out + r0 * patch);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <class Starts>
hipError_t launch_blend(const float* patches, int B, int Dc, int H, int W, int res, const Starts& s, bool v4,
                        const double* tables, float* out, hipStream_t st) {
    const int per_plane = H * (W / (v4 ? 4 : 1));
    const dim3 grid((per_plane + 255) / 256, Dc, B);
    const auto kernel = v4 ? patch_blend_kernel<4, Starts> : patch_blend_kernel<1, Starts>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, patches, B, Dc, H, W, res, s, tables, out);
    return hipGetLastError();
}

}  // namespace

// at most DDPM3D_JOINT_MAX_STARTS^3 * DDPM3D_MAX_DRAWS = 8^3 * 64 = 32768 rows: always one launch
hipError_t ddpm3d_launch_joint_gather(const float* canvas, int B, int Dc, int H, int W, int res,
                                      const ddpm3d_joint_starts& s, int first_patch, int n_patches, float* out,
                                      hipStream_t st) {
    const bool v4 = quads(s.ny, s.ys, W, res) && aligned16(canvas) && aligned16(out);
    return launch_gather(canvas, B, Dc, H, W, res, StartsByValue{s}, v4, (int64_t)first_patch * B,
                         (int64_t)n_patches * B, out, st);
}

hipError_t ddpm3d_launch_joint_blend(const float* patches, int B, int Dc, int H, int W, int res,
                                     const ddpm3d_joint_starts& s, const double* tables, float* out, hipStream_t st) {
    const bool v4 = quads(s.ny, s.ys, W, res) && aligned16(patches) && aligned16(out);
    return launch_blend(patches, B, Dc, H, W, res, StartsByValue{s}, v4, tables, out, st);
}

hipError_t ddpm3d_launch_tiles_gather(const float* canvas, int B, int Dc, int H, int W, int res,
                                      const ddpm3d_tiling& t, int first_patch, int n_patches, float* out,
                                      hipStream_t st) {
    const bool v4 = quads(t.n[1], t.starts[1], W, res) && aligned16(canvas) && aligned16(out);
    return launch_gather(canvas, B, Dc, H, W, res, StartsInMemory{t.n[0], t.n[1], t.n[2], t.d_starts, t.d_cover}, v4,
                         (int64_t)first_patch * B, (int64_t)n_patches * B, out, st);
}

hipError_t ddpm3d_launch_tiles_blend(const float* patches, int B, int Dc, int H, int W, int res,
                                     const ddpm3d_tiling& t, float* out, hipStream_t st) {
    const bool v4 = quads(t.n[1], t.starts[1], W, res) && aligned16(patches) && aligned16(out);
    return launch_blend(patches, B, Dc, H, W, res, StartsInMemory{t.n[0], t.n[1], t.n[2], t.d_starts, t.d_cover}, v4,
                        t.d_tables, out, st);
}
