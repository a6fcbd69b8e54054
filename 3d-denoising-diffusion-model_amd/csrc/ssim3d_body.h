// The march of the 3-D SSIM, shared by ssim3d_kernel (metrics.hip) and the per-scale kernel of the
// multi-scale SSIM (msssim.hip): one body templated on whether the contrast-structure term CS gets
// a sum of its own.  Both kernels evaluate S by the same expression in the same order, so scale 0 of the multi-scale
// entry carries the bits of ddpm3d_ssim3d.  The records and their fold are record_reduce.h's, every column a sum; the
// map is written with one float per lane: no wide store whose data registers could be rewritten behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "record_reduce.h"

namespace {

// A workgroup owns a 16 (h) x 32 (w) tile of interior voxels and marches along d through one chunk of the depth.
// Per input plane: the tile plus its halo of 10 of both volumes goes to LDS with a pivot taken off, the five
// fields x, y, x^2, y^2, xy are filtered along w into a second LDS image, each thread filters its two outputs
// along h and feeds the five values into the d filter, held in registers as the ten unfinished sums per field:
// a plane adds w[j] * v to the outputs in flight and finishes the oldest, which is combined into S, written to
// the map and added to the thread's fp64 sum.  Nothing but the map goes back to HBM.
constexpr int SS_TW = 32, SS_TH = 16, SS_R = 5, SS_TAPS = 2 * SS_R + 1;
constexpr int SS_THREADS = 256;
constexpr int SS_IW = SS_TW + 2 * SS_R, SS_IH = SS_TH + 2 * SS_R;     // 42 x 26 inputs per plane
constexpr int SS_IN = SS_IW * SS_IH;
constexpr int SS_LOADS = (SS_IN + SS_THREADS - 1) / SS_THREADS;       // 5 per thread and volume
constexpr int SS_ROWITEMS = SS_IH * SS_TW;                            // 832 row-filtered points per field
constexpr int SS_OUT = SS_TW * SS_TH / SS_THREADS;                    // 2 outputs per thread, SS_TH / 2 rows apart
constexpr int SS_FIELDS = 5;
constexpr int SS_MIN_CHUNK = 16;           // output planes per chunk at least: a chunk pays 10 warm-up planes
constexpr int SS_TARGET_WGS = 1024;        // per estimate: 4 workgroups per CU

struct SsTaps {
    float w[SS_TAPS];
};
// skimage's window: exp(-0.5 (j - 5)^2 / sigma^2), sigma = 1.5, normalised to sum 1 in fp64, then rounded
inline SsTaps ss_taps() {
    SsTaps taps;
    double g[SS_TAPS], tot = 0.0;
    for (int j = 0; j < SS_TAPS; ++j) tot += g[j] = exp(-0.5 * (j - SS_R) * (j - SS_R) / (1.5 * 1.5));
    for (int j = 0; j < SS_TAPS; ++j) taps.w[j] = (float)(g[j] / tot);
    return taps;
}

struct SsPlan {
    int tiles_w, tiles_h, chunks, chunk;   // chunk = output planes per chunk
};
inline SsPlan ss_plan(int D, int H, int W) {
    SsPlan p;
    const int od = D - 2 * SS_R;
    p.tiles_w = (W - 2 * SS_R + SS_TW - 1) / SS_TW;
    p.tiles_h = (H - 2 * SS_R + SS_TH - 1) / SS_TH;
    const int64_t tiles = (int64_t)p.tiles_w * p.tiles_h;
    int64_t want = (SS_TARGET_WGS + tiles - 1) / tiles;
    const int most = (od + SS_MIN_CHUNK - 1) / SS_MIN_CHUNK;
    if (want > most) want = most;
    p.chunk = (int)((od + want - 1) / want);
    p.chunks = (od + p.chunk - 1) / p.chunk;
    return p;
}
// records the workspace holds per estimate: an upper bound of tiles * chunks that grows with every extent
inline int64_t ss_records(int D, int H, int W) {
    const SsPlan p = ss_plan(D, H, W);
    return (int64_t)p.tiles_w * p.tiles_h * ((D - 2 * SS_R + SS_MIN_CHUNK - 1) / SS_MIN_CHUNK);
}

// doubles per record: {sum S, count}, or {sum S, sum CS, count} with the contrast-structure term
template <bool CS>
constexpr int SS_REC = CS ? 3 : 2;

// The body of a kernel of SS_THREADS threads on a grid (tiles, chunks, B).  CS: also sums
// (2 s_xy + C2) / (s_x + s_y + C2) over the counted voxels.
template <bool CS>
__device__ __forceinline__ void ssim3d_march(
    const float* __restrict__ est, const float* __restrict__ target, const uint8_t* __restrict__ mask, int D, int H,
    int W, float C1, float C2, const SsTaps& taps, int chunk, int64_t recs, float* __restrict__ map,
    double* __restrict__ ws) {
    constexpr int REC = SS_REC<CS>;
    __shared__ float tile[2][SS_IH][SS_IW];
    __shared__ float rowf[SS_FIELDS][SS_IH][SS_TW];
    __shared__ float pmin[2][SS_THREADS / 64];

    const int tid = threadIdx.x, tx = tid % SS_TW, ty = tid / SS_TW;
    const int tiles_w = (W - 2 * SS_R + SS_TW - 1) / SS_TW;
    const int ow0 = (blockIdx.x % tiles_w) * SS_TW, oh0 = (blockIdx.x / tiles_w) * SS_TH;
    const int OD = D - 2 * SS_R, OH = H - 2 * SS_R, OW = W - 2 * SS_R;
    const int od0 = blockIdx.y * chunk;
    const int od1 = od0 + chunk < OD ? od0 + chunk : OD;
    const int b = blockIdx.z;
    const int64_t plane = (int64_t)H * W;
    const float* __restrict__ xb = est + (int64_t)b * D * plane;

    // this thread's share of a plane's inputs: offsets inside the plane, -1 outside the volume
    int off[SS_LOADS];
#pragma unroll
    for (int i = 0; i < SS_LOADS; ++i) {
        const int e = tid + i * SS_THREADS;
        const int ih = oh0 + e / SS_IW, iw = ow0 + e % SS_IW;
        off[i] = (e < SS_IN && ih < H && iw < W) ? ih * W + iw : -1;
    }
    float px[SS_LOADS], py[SS_LOADS];
    auto fetch = [&](int d) {
        const int64_t base = (int64_t)d * plane;
#pragma unroll
        for (int i = 0; i < SS_LOADS; ++i) {
            px[i] = off[i] >= 0 ? xb[base + off[i]] : INFINITY;
            py[i] = off[i] >= 0 ? target[base + off[i]] : INFINITY;
        }
    };
    const int planes = od1 - od0 + 2 * SS_R;

    // The pivots: each volume's own minimum over the first, middle and last plane of this workgroup's block.  A value
    // inside the block would do for data on an offset, but PET volumes are flat where they are lowest (the
    // background), and there, where the variances are smallest, (mean - pivot)^2 must be smallest too.  Nothing of
    // another estimate enters, so a batched call gives the bits of single calls; a constant volume has variance 0.
    float pvx = INFINITY, pvy = INFINITY;
    for (int k = 0; k < 3; ++k) {
        fetch(od0 + (k * (planes - 1)) / 2);
#pragma unroll
        for (int i = 0; i < SS_LOADS; ++i) {
            pvx = fminf(pvx, px[i]);
            pvy = fminf(pvy, py[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pvx = fminf(pvx, __shfl_xor(pvx, o));
        pvy = fminf(pvy, __shfl_xor(pvy, o));
    }
    if ((tid & 63) == 0) { pmin[0][tid >> 6] = pvx; pmin[1][tid >> 6] = pvy; }
    __syncthreads();
    pvx = fminf(fminf(pmin[0][0], pmin[0][1]), fminf(pmin[0][2], pmin[0][3]));
    pvy = fminf(fminf(pmin[1][0], pmin[1][1]), fminf(pmin[1][2], pmin[1][3]));

    float acc[SS_OUT][SS_FIELDS][SS_TAPS - 1];
#pragma unroll
    for (int o = 0; o < SS_OUT; ++o)
#pragma unroll
        for (int f = 0; f < SS_FIELDS; ++f)
#pragma unroll
            for (int k = 0; k < SS_TAPS - 1; ++k) acc[o][f][k] = 0.0f;
    double sum = 0.0, sum_cs = 0.0;
    unsigned count = 0;

    fetch(od0);
    for (int r = 0; r < planes; ++r) {
        // (the previous plane's row pass, the readers of `tile`, ended before that plane's second barrier)
#pragma unroll
        for (int i = 0; i < SS_LOADS; ++i) {
            const int e = tid + i * SS_THREADS;
            if (e < SS_IN) {
                (&tile[0][0][0])[e] = off[i] >= 0 ? px[i] - pvx : 0.0f;      // outside the volume: no output reads it
                (&tile[1][0][0])[e] = off[i] >= 0 ? py[i] - pvy : 0.0f;
            }
        }
        __syncthreads();
        if (r + 1 < planes) fetch(od0 + r + 1);            // in flight behind this plane's arithmetic

        // along w
        for (int e = tid; e < SS_ROWITEMS; e += SS_THREADS) {
            const int row = e / SS_TW, col = e % SS_TW;
            float s[SS_FIELDS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < SS_TAPS; ++j) {
                const float xv = tile[0][row][col + j], yv = tile[1][row][col + j], wj = taps.w[j];
                const float wx = wj * xv, wy = wj * yv;
                s[0] += wx;
                s[1] += wy;
                s[2] += wx * xv;
                s[3] += wy * yv;
                s[4] += wx * yv;
            }
#pragma unroll
            for (int f = 0; f < SS_FIELDS; ++f) rowf[f][row][col] = s[f];
        }
        __syncthreads();

        // along h, then into the d filter
        const bool emit = r >= 2 * SS_R;
        const int od = od0 + r - 2 * SS_R;
#pragma unroll
        for (int o = 0; o < SS_OUT; ++o) {
            const int lh = ty + o * (SS_TH / SS_OUT);
            float v[SS_FIELDS];
#pragma unroll
            for (int f = 0; f < SS_FIELDS; ++f) {
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < SS_TAPS; ++j) s += taps.w[j] * rowf[f][lh + j][tx];
                v[f] = s;
            }
            float done[SS_FIELDS];
#pragma unroll
            for (int f = 0; f < SS_FIELDS; ++f) {
                done[f] = acc[o][f][0] + taps.w[SS_TAPS - 1] * v[f];
#pragma unroll
                for (int k = 0; k < SS_TAPS - 2; ++k) acc[o][f][k] = acc[o][f][k + 1] + taps.w[SS_TAPS - 2 - k] * v[f];
                acc[o][f][SS_TAPS - 2] = taps.w[0] * v[f];
            }
            const int oh = oh0 + lh, ow = ow0 + tx;
            if (emit && oh < OH && ow < OW) {
                // un-pivot the means; variances and covariance of pivoted values are those of the values
                const float mx = done[0], my = done[1];
                const float vx = done[2] - mx * mx, vy = done[3] - my * my, vxy = done[4] - mx * my;
                const float ux = pvx + mx, uy = pvy + my;
                const float num = (2.0f * ux * uy + C1) * (2.0f * vxy + C2);
                const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
                const float S = num / den;
                const int64_t oidx = ((int64_t)od * OH + oh) * OW + ow;
                if (map) map[(int64_t)b * OD * OH * OW + oidx] = S;
                const bool on = mask ? mask[(int64_t)(od + SS_R) * plane + (int64_t)(oh + SS_R) * W + (ow + SS_R)] != 0
                                     : true;
                if (on) {
                    sum += (double)S;
                    if constexpr (CS) sum_cs += (double)((2.0f * vxy + C2) / (vx + vy + C2));
                    count += 1;
                }
            }
        }
    }

    double tot[REC];
    tot[0] = sum;
    if constexpr (CS) tot[1] = sum_cs;
    tot[REC - 1] = (double)count;
    rr_write_record<RrSum<REC>, SS_THREADS>(
        tot, ws + ((int64_t)b * recs + (int64_t)blockIdx.y * gridDim.x + blockIdx.x) * REC);
}

// The body of the fold kernel, 256 threads, one workgroup per estimate: the columns of its `used` records of REC
// doubles in a fixed order, written to out[b * out_stride ..].
template <int REC>
__device__ __forceinline__ void ssim3d_fold(const double* __restrict__ ws, int64_t recs, int used,
                                            double* __restrict__ out, int out_stride) {
    const int b = blockIdx.x;
    rr_fold_record<RrSum<REC>, 256>(ws + (int64_t)b * recs * REC, used, out + (size_t)b * out_stride);
}

}  // namespace
