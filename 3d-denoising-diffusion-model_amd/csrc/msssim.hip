// Multi-scale 3-D SSIM (Wang, Simoncelli, Bovik 2003; definitions in include/ddpm3d.h): a streaming
// 2 x 2 x 2 mean pooling of B volumes and their mask, the march of ssim3d_kernel (ssim3d_body.h) with the
// contrast-structure term as a sum of its own, and the driver that runs them scale by scale into the caller's
// workspace.  Enqueue-only: no allocation, no synchronisation, no floating-point atomics.  Offsets are 64-bit; the
// pooled volume is written one float per lane, the pooled mask one byte per lane, the records as halves of doubles.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "ssim3d_body.h"

namespace {

// ------------------------------------------------------------------------------------------------ pooling
// A workgroup of 64 (w) x 4 (h) threads writes that tile of one output plane; a thread reads its 2 x 2 x 2 inputs
// (WIDE: as four 8-byte loads, a wave then reads 512 contiguous bytes of each of its four rows) and sums them in the
// one order the header fixes, so that both paths give the same bits.  The workgroups of volume 0 also pool the mask.
constexpr int PL_TW = 64, PL_TH = 4;

template <bool WIDE>
__global__ __launch_bounds__(PL_TW * PL_TH) void pool2_kernel(
    const float* __restrict__ vol, const uint8_t* __restrict__ mask, int D, int H, int W, int tiles_w, int tiles_h,
    float* __restrict__ out, uint8_t* __restrict__ mask_out) {
    const int OD = D >> 1, OH = H >> 1, OW = W >> 1;
    const int tw = blockIdx.x % tiles_w, rest = blockIdx.x / tiles_w;
    const int th = rest % tiles_h, od = rest / tiles_h;
    const int ow = tw * PL_TW + threadIdx.x, oh = th * PL_TH + threadIdx.y;
    if (ow >= OW || oh >= OH || od >= OD) return;
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)H * W;
    const int64_t in0 = ((int64_t)(2 * od) * H + 2 * oh) * W + 2 * ow;       // voxel (2 od, 2 oh, 2 ow)
    const float* __restrict__ src = vol + (int64_t)b * D * plane + in0;
    float v[2][2][2];                                                       // [dz][dy][dx]
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const float* __restrict__ row = src + dz * plane + (int64_t)dy * W;
            if constexpr (WIDE) {
                const float2 p = *reinterpret_cast<const float2*>(row);
                v[dz][dy][0] = p.x, v[dz][dy][1] = p.y;
            } else {
                v[dz][dy][0] = row[0], v[dz][dy][1] = row[1];
            }
        }
    const float sum = ((v[0][0][0] + v[0][0][1]) + (v[0][1][0] + v[0][1][1])) +
                      ((v[1][0][0] + v[1][0][1]) + (v[1][1][0] + v[1][1][1]));
    const int64_t o = ((int64_t)od * OH + oh) * OW + ow;
    out[(int64_t)b * OD * OH * OW + o] = sum * 0.125f;
    if (mask && b == 0) {
        const uint8_t* __restrict__ m = mask + in0;
        int n = 0;
#pragma unroll
        for (int dz = 0; dz < 2; ++dz)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const uint8_t* __restrict__ row = m + dz * plane + (int64_t)dy * W;
                n += (row[0] != 0) + (row[1] != 0);
            }
        mask_out[o] = n >= 4 ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------ per-scale SSIM parts
__global__ __launch_bounds__(SS_THREADS) void msssim3d_parts_kernel(
    const float* __restrict__ est, const float* __restrict__ target, const uint8_t* __restrict__ mask, int D, int H,
    int W, float C1, float C2, SsTaps taps, int chunk, int64_t recs, double* __restrict__ ws) {
    ssim3d_march<true>(est, target, mask, D, H, W, C1, C2, taps, chunk, recs, nullptr, ws);
}

// One workgroup per estimate: {sum S, sum CS, count} over its `used` records in a fixed order, to the scale's
// triple of out[B][scales][3].
__global__ __launch_bounds__(256) void msssim3d_fold_kernel(const double* __restrict__ ws, int64_t recs, int used,
                                                            double* __restrict__ out, int out_stride) {
    ssim3d_fold<3>(ws, recs, used, out, out_stride);
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

// The workspace: the records of one scale (scale 0's are the most), then per scale j >= 1 the pooled estimates,
// the pooled target and the pooled mask, every block 16-byte aligned.
struct MsLayout {
    size_t est[DDPM3D_MSSSIM_MAX_SCALES], target[DDPM3D_MSSSIM_MAX_SCALES], mask[DDPM3D_MSSSIM_MAX_SCALES], bytes;
};
MsLayout ms_layout(int B, int D, int H, int W, int scales) {
    MsLayout l = {};
    size_t at = round16((size_t)B * (size_t)ss_records(D, H, W) * 3 * sizeof(double));
    for (int j = 1; j < scales; ++j) {
        const size_t voxels = (size_t)(D >> j) * (size_t)(H >> j) * (size_t)(W >> j);
        l.est[j] = at, at += round16((size_t)B * voxels * sizeof(float));
        l.target[j] = at, at += round16(voxels * sizeof(float));
        l.mask[j] = at, at += round16(voxels);
    }
    l.bytes = at;
    return l;
}

}  // namespace

hipError_t ddpm3d_launch_pool2(const float* vol, const uint8_t* mask, int B, int D, int H, int W, float* out,
                               uint8_t* mask_out, hipStream_t st) {
    const int OD = D >> 1, OH = H >> 1, OW = W >> 1;
    const int tiles_w = (OW + PL_TW - 1) / PL_TW, tiles_h = (OH + PL_TH - 1) / PL_TH;
    const dim3 grid((unsigned)((int64_t)tiles_w * tiles_h * OD), B), block(PL_TW, PL_TH);
    // with W even every row of every volume starts on a multiple of 8 bytes from the base
    if (W % 2 == 0 && aligned(vol, 8))
        hipLaunchKernelGGL(pool2_kernel<true>, grid, block, 0, st, vol, mask, D, H, W, tiles_w, tiles_h, out, mask_out);
    else
        hipLaunchKernelGGL(pool2_kernel<false>, grid, block, 0, st, vol, mask, D, H, W, tiles_w, tiles_h, out,
                           mask_out);
    return hipGetLastError();
}

size_t ddpm3d_ms_workspace_bytes(int B, int D, int H, int W, int scales) { return ms_layout(B, D, H, W, scales).bytes; }

hipError_t ddpm3d_launch_msssim3d(const float* est, const float* target, const uint8_t* mask, int B, int D, int H,
                                  int W, int scales, float C1, float C2, void* ws, double* out, hipStream_t st) {
    const MsLayout l = ms_layout(B, D, H, W, scales);
    const SsTaps taps = ss_taps();
    char* base = static_cast<char*>(ws);
    double* records = static_cast<double*>(ws);
    for (int j = 0; j < scales; ++j) {
        const int Dj = D >> j, Hj = H >> j, Wj = W >> j;
        const SsPlan p = ss_plan(Dj, Hj, Wj);
        const int64_t recs = ss_records(Dj, Hj, Wj);
        const int tiles = p.tiles_w * p.tiles_h;
        hipLaunchKernelGGL(msssim3d_parts_kernel, dim3(tiles, p.chunks, B), dim3(SS_THREADS), 0, st, est, target, mask,
                           Dj, Hj, Wj, C1, C2, taps, p.chunk, recs, records);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(msssim3d_fold_kernel, dim3(B), dim3(256), 0, st, records, recs, tiles * p.chunks,
                           out + (size_t)j * 3, scales * 3);
        e = hipGetLastError();
        if (e != hipSuccess || j + 1 == scales) return e;
        float* est_next = reinterpret_cast<float*>(base + l.est[j + 1]);
        float* target_next = reinterpret_cast<float*>(base + l.target[j + 1]);
        uint8_t* mask_next = mask ? reinterpret_cast<uint8_t*>(base + l.mask[j + 1]) : nullptr;
        e = ddpm3d_launch_pool2(est, nullptr, B, Dj, Hj, Wj, est_next, nullptr, st);
        if (e != hipSuccess) return e;
        e = ddpm3d_launch_pool2(target, mask, 1, Dj, Hj, Wj, target_next, mask_next, st);
        if (e != hipSuccess) return e;
        est = est_next, target = target_next, mask = mask_next;
    }
    return hipSuccess;
}
