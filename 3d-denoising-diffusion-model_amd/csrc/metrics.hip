// Image-quality metrics of an estimate against a full-dose target volume (definitions in
// include/ddpm3d.h).  Both entries reduce B estimates against one shared target in one launch plus a fold:
// every workgroup writes one fp64 record to the caller's workspace and a second, small launch folds a volume's
// records in a fixed order.  No floating-point atomics: the same bits on every run.  Offsets are 64-bit
// (B * voxels passes 2^31 for 16 whole-body draws).  Records are written with 4-byte stores (halves of the
// doubles), the map with one float per lane: no wide store whose data registers could be rewritten behind it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ void store_double(double* p, int lane_half, double v) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    reinterpret_cast<unsigned*>(p)[lane_half] = lane_half ? (unsigned)(bits >> 32) : (unsigned)bits;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ------------------------------------------------------------------------------------------- error moments
constexpr int EM_THREADS = 256;
constexpr int EM_VEC = 4;
constexpr int EM_MAX_PARTS = 2048;         // 8 workgroups per CU: enough loads in flight to stream from HBM
constexpr int EM_REC = DDPM3D_EM_REC;

// Folds the ten per-thread values over the workgroup (sums in columns 0..5 and 8..9, min / max in 6 / 7), each in
// a fixed order, and has lanes 0..19 write the record.
__device__ __forceinline__ void em_write_record(double (&v)[EM_REC], double* __restrict__ rec) {
    __shared__ double red[EM_REC][EM_THREADS / 64];
#pragma unroll
    for (int k = 0; k < EM_REC; ++k)
        v[k] = k == DDPM3D_EM_MIN_Y ? wave_min(v[k]) : k == DDPM3D_EM_MAX_Y ? wave_max(v[k]) : wave_sum(v[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < EM_REC; ++k) red[k][wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 2 * EM_REC) {
        const int k = threadIdx.x >> 1;
        double tot = red[k][0];
        for (int w = 1; w < EM_THREADS / 64; ++w)
            tot = k == DDPM3D_EM_MIN_Y ? fmin(tot, red[k][w]) : k == DDPM3D_EM_MAX_Y ? fmax(tot, red[k][w])
                                                                                  : tot + red[k][w];
        store_double(rec + k, threadIdx.x & 1, tot);
    }
}

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
    em_write_record(rec, ws + ((size_t)b * parts + part) * EM_REC);
}

// One workgroup per estimate: its records in a fixed order.
__global__ __launch_bounds__(EM_THREADS) void error_moments_fold_kernel(const double* __restrict__ ws, int parts,
                                                                        double* __restrict__ out) {
    const int b = blockIdx.x;
    double rec[EM_REC];
#pragma unroll
    for (int k = 0; k < EM_REC; ++k) rec[k] = 0.0;
    rec[DDPM3D_EM_MIN_Y] = INFINITY;
    rec[DDPM3D_EM_MAX_Y] = -INFINITY;
    for (int p = threadIdx.x; p < parts; p += EM_THREADS) {
        const double* r = ws + ((size_t)b * parts + p) * EM_REC;
#pragma unroll
        for (int k = 0; k < EM_REC; ++k)
            rec[k] = k == DDPM3D_EM_MIN_Y ? fmin(rec[k], r[k]) : k == DDPM3D_EM_MAX_Y ? fmax(rec[k], r[k])
                                                                                  : rec[k] + r[k];
    }
    em_write_record(rec, out + (size_t)b * EM_REC);
}

struct EmPlan {
    int parts;
    int64_t chunk;
};
EmPlan em_plan(int64_t voxels) {
    const int64_t per = EM_THREADS * EM_VEC;
    const int64_t passes = (voxels + per - 1) / per;
    const int parts = (int)(passes < EM_MAX_PARTS ? passes : EM_MAX_PARTS);
    const int64_t chunk = (passes + parts - 1) / parts * per;
    return {(int)((voxels + chunk - 1) / chunk), chunk};
}

// ---------------------------------------------------------------------------------------------- 3-D SSIM
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

struct SsPlan {
    int tiles_w, tiles_h, chunks, chunk;   // chunk = output planes per chunk
};
SsPlan ss_plan(int D, int H, int W) {
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
int64_t ss_records(int D, int H, int W) {
    const SsPlan p = ss_plan(D, H, W);
    return (int64_t)p.tiles_w * p.tiles_h * ((D - 2 * SS_R + SS_MIN_CHUNK - 1) / SS_MIN_CHUNK);
}

__global__ __launch_bounds__(SS_THREADS) void ssim3d_kernel(
    const float* __restrict__ est, const float* __restrict__ target, const uint8_t* __restrict__ mask, int D, int H,
    int W, float C1, float C2, SsTaps taps, int chunk, int64_t recs, float* __restrict__ map,
    double* __restrict__ ws) {
    __shared__ float tile[2][SS_IH][SS_IW];
    __shared__ float rowf[SS_FIELDS][SS_IH][SS_TW];
    __shared__ double red[2][SS_THREADS / 64];
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
    double sum = 0.0;
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
                    count += 1;
                }
            }
        }
    }

    sum = wave_sum(sum);
    double cnt = wave_sum((double)count);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) { red[0][wave] = sum; red[1][wave] = cnt; }
    __syncthreads();
    if (tid < 4) {
        const int k = tid >> 1;
        const double tot = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
        double* rec = ws + ((int64_t)b * recs + (int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        store_double(rec + k, tid & 1, tot);
    }
}

// One workgroup per estimate: {sum S, count} over its `used` records in a fixed order.
__global__ __launch_bounds__(256) void ssim3d_fold_kernel(const double* __restrict__ ws, int64_t recs, int used,
                                                          double* __restrict__ out) {
    __shared__ double red[2][4];
    const int b = blockIdx.x;
    double s = 0.0, c = 0.0;
    for (int p = threadIdx.x; p < used; p += 256) {
        const double* r = ws + ((int64_t)b * recs + p) * 2;
        s += r[0];
        c += r[1];
    }
    s = wave_sum(s);
    c = wave_sum(c);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = s; red[1][wave] = c; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x >> 1;
        const double tot = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
        store_double(out + (size_t)b * 2 + k, threadIdx.x & 1, tot);
    }
}

}  // namespace

// an upper bound of the records a launch writes that never shrinks as the volume grows
size_t ddpm3d_em_workspace_bytes(int B, int64_t voxels) {
    const int64_t per = EM_THREADS * EM_VEC, passes = (voxels + per - 1) / per;
    return (size_t)B * (size_t)(passes < EM_MAX_PARTS ? passes : EM_MAX_PARTS) * EM_REC * sizeof(double);
}

hipError_t ddpm3d_launch_error_moments(const float* est, const float* target, const uint8_t* mask, const float* std,
                                       int B, int64_t voxels, double* ws, double* out, hipStream_t st) {
    const EmPlan p = em_plan(voxels);
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
    // skimage's window: exp(-0.5 (j - 5)^2 / sigma^2), sigma = 1.5, normalised to sum 1 in fp64, then rounded
    SsTaps taps;
    double g[SS_TAPS], tot = 0.0;
    for (int j = 0; j < SS_TAPS; ++j) tot += g[j] = exp(-0.5 * (j - SS_R) * (j - SS_R) / (1.5 * 1.5));
    for (int j = 0; j < SS_TAPS; ++j) taps.w[j] = (float)(g[j] / tot);
    const int64_t recs = ss_records(D, H, W);
    const int tiles = p.tiles_w * p.tiles_h;
    hipLaunchKernelGGL(ssim3d_kernel, dim3(tiles, p.chunks, B), dim3(SS_THREADS), 0, st, est, target, mask, D, H, W,
                       C1, C2, taps, p.chunk, recs, map, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssim3d_fold_kernel, dim3(B), dim3(256), 0, st, ws, recs, tiles * p.chunks, out);
    return hipGetLastError();
}
