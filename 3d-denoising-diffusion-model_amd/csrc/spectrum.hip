// Windowed 3-D DFT of fp32 volumes as three dense per-axis GEMMs on the exact fp32-input MFMA, and the per-shell sums
// of the result (definitions in include/ddpm3d.h).
//   dft_gemm_kernel<PASS_W>: one LDS-tiled GEMM C[M][N] = A[M][K] B[K][N] per pass.  Pass W (real -> complex): A is
//     the volume's rows minus the pivot (K = x contiguous), B the transposed [C; S] table (K contiguous again), N =
//     2 Wh.  Passes H and D (complex -> complex as one real GEMM, K = 2n): A is [C | -S; S | C] built from the two
//     tables in the operand load, B is [Xr; Xi] with N (= kw, or h * Wh + kw) contiguous.  Either way the lanes of a
//     store run along contiguous memory.
//   sp_chunk_kernel / sp_fold_kernel: roi.hip's frame over a shell index of half-spectrum coefficients, with the twin
//     weight from index % Wh.  The reduction is record_reduce.h's: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "record_reduce.h"

namespace {

// ---------------------------------------------------------------------------------------------- the GEMM
constexpr int DFT_THREADS = 256;
constexpr int BM = 128, BN = 128, BK = 16;     // workgroup tile; a wave owns 64 x 64 as 2 x 2 MFMA tiles of 32 x 32
constexpr int LDS_ROW = BM + 32;               // k rows 32 banks apart: the two k of one MFMA step never collide
static_assert(BM == BN && BK % 2 == 0 && DFT_THREADS == 256, "the load maps below are written for this tile");
using f32x16 = __attribute__((ext_vector_type(16))) float;

struct DftPass {
    const float* cos_t;     // [R][n]
    const float* sin_t;     // [R][n]
    int n, R;               // transform length, table rows
    int64_t M;              // pass W: B * D * H volume rows; else 2 R
    int N, K;               // pass W: 2 Wh, W; else the columns per batch and 2 n
    int64_t mtiles;
    int ntiles;
    const float* in_re;     // pass W: the volumes; else plane [batch][n][N]
    const float* in_im;
    float* out_re;          // pass W: [M][R]; else [batch][R][N]
    float* out_im;
    const float* pivot;     // pass W: [B] or NULL
    int rows_per_volume;    // pass W: D * H
};

// element (row, k) of [C; S] (k < n) or of [C | -S; S | C]; row < 2 R and k < K are the caller's
__device__ __forceinline__ float twiddle(const DftPass& p, int row, int k) {
    const bool im_row = row >= p.R, im_col = k >= p.n;
    const int r = im_row ? row - p.R : row, x = im_col ? k - p.n : k;
    const float v = (im_row == im_col ? p.cos_t : p.sin_t)[(int64_t)r * p.n + x];
    return (!im_row && im_col) ? -v : v;
}

template <bool PASS_W>
__global__ __launch_bounds__(DFT_THREADS) void dft_gemm_kernel(const DftPass p) {
    __shared__ float As[2][BK][LDS_ROW], Bs[2][BK][LDS_ROW];      // two stages: one barrier per k tile
    const int t = threadIdx.x;
    int64_t tile = blockIdx.x;
    const int n0 = (int)(tile % p.ntiles) * BN;
    tile /= p.ntiles;
    const int64_t m0 = (tile % p.mtiles) * BM;
    const int64_t batch = tile / p.mtiles;

    // K-contiguous operands: thread t takes k = t & 15 of rows (t >> 4) + 16 j; the N-contiguous one: columns
    // (t & 31) + 32 i of k = (t >> 5) + 8 j
    const int kc = t & 15, rc = t >> 4;
    const int nc = t & 31, kn = t >> 5;
    float pv[8];
    if constexpr (PASS_W) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t m = m0 + rc + 16 * j;
            pv[j] = (p.pivot && m < p.M) ? p.pivot[m / p.rows_per_volume] : 0.0f;
        }
    }
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
        const int k = k0 + kc;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t m = m0 + rc + 16 * j;
            float a = 0.0f;
            if (m < p.M && k < p.K) {
                if constexpr (PASS_W) a = p.in_re[m * p.K + k] - pv[j];
                else a = twiddle(p, (int)m, k);
            }
            ra[j] = a;
        }
        if constexpr (PASS_W) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = n0 + rc + 16 * j;
                rb[j] = (col < p.N && k < p.K) ? twiddle(p, col, k) : 0.0f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int kk = k0 + kn + 8 * j;
                const bool im = kk >= p.n;
                const float* __restrict__ row =
                    (im ? p.in_im : p.in_re) + (batch * p.n + (im ? kk - p.n : kk)) * (int64_t)p.N;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int col = n0 + nc + 32 * i;
                    rb[j * 4 + i] = (kk < p.K && col < p.N) ? row[col] : 0.0f;
                }
            }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 8; ++j) As[buf][kc][rc + 16 * j] = ra[j];
        if constexpr (PASS_W) {
#pragma unroll
            for (int j = 0; j < 8; ++j) Bs[buf][kc][rc + 16 * j] = rb[j];
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) Bs[buf][kn + 8 * j][nc + 32 * i] = rb[j * 4 + i];
        }
    };

    const int wave = t >> 6, lane = t & 63;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    fetch(0);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < p.K; k0 += BK, buf ^= 1) {
        const bool more = k0 + BK < p.K;
        if (more) fetch(k0 + BK);                  // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a0 = As[buf][kk + lh][wm + lr], a1 = As[buf][kk + lh][wm + 32 + lr];
            const float b0 = Bs[buf][kk + lh][wn + lr], b1 = Bs[buf][kk + lh][wn + 32 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) stage(buf ^ 1);                  // the other stage: its readers left it before the last barrier
        __syncthreads();
    }

    // D layout of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  4-byte stores
    // whose lanes run along the contiguous dimension.
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn + 32 * j + lr;
            if (col >= p.N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= p.M) continue;
                if constexpr (PASS_W) {
                    const bool im = col >= p.R;
                    (im ? p.out_im : p.out_re)[m * p.R + (im ? col - p.R : col)] = acc[i][j][r];
                } else {
                    const bool im = m >= p.R;
                    (im ? p.out_im : p.out_re)[(batch * p.R + (im ? m - p.R : m)) * (int64_t)p.N + col] = acc[i][j][r];
                }
            }
        }
}

template <bool PASS_W>
hipError_t launch_pass(DftPass p, int64_t batches, hipStream_t st) {
    p.mtiles = (p.M + BM - 1) / BM;
    p.ntiles = (p.N + BN - 1) / BN;
    const int64_t tiles = batches * p.mtiles * p.ntiles;    // at most 2^28 / 128 * 17 in pass W, fewer elsewhere
    hipLaunchKernelGGL(dft_gemm_kernel<PASS_W>, dim3((unsigned)tiles), dim3(DFT_THREADS), 0, st, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the shell sums
constexpr int SP_THREADS = 256;
constexpr int SP_PER = DDPM3D_ROI_CHUNK / SP_THREADS;
static_assert(DDPM3D_ROI_CHUNK % SP_THREADS == 0, "a chunk is a whole number of passes");
using SpCols = RrSum<DDPM3D_SP_REC - 1, DDPM3D_SP_REC>;

// Workgroup (c, b), as roi_chunk_kernel: chunk c belongs to the shell s with chunks[s] <= c < chunks[s + 1].  An index
// value outside [0, coeffs) is skipped, so no load leaves the spectra.
__global__ __launch_bounds__(SP_THREADS) void sp_chunk_kernel(
    const float* __restrict__ xre, const float* __restrict__ xim, const float* __restrict__ yre,
    const float* __restrict__ yim, int64_t coeffs, int W, int Wh, int S, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ chunks, const int64_t* __restrict__ index, int64_t total, double* __restrict__ ws) {
    // squares of fp32 values are exact in fp64; the sums of two of them and the running sums round one at a time
#pragma clang fp contract(off)
    const int64_t c = blockIdx.x;
    const int b = blockIdx.y;
    int lo = 0, hi = S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunks[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t e0 = offsets[lo] + (c - chunks[lo]) * DDPM3D_ROI_CHUNK;
    const int64_t end = offsets[lo + 1];
    const int64_t e1 = e0 + DDPM3D_ROI_CHUNK < end ? e0 + DDPM3D_ROI_CHUNK : end;
    const float* __restrict__ xr = xre + (int64_t)b * coeffs;
    const float* __restrict__ xi = xim + (int64_t)b * coeffs;

    int64_t at[SP_PER];
#pragma unroll
    for (int j = 0; j < SP_PER; ++j) {
        const int64_t e = e0 + threadIdx.x + j * SP_THREADS;
        const int64_t v = e < e1 ? index[e] : -1;
        at[j] = v < coeffs ? v : -1;
    }
    double n = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0, see = 0.0;
#pragma unroll
    for (int j = 0; j < SP_PER; ++j) {
        if (at[j] < 0) continue;
        const int kw = (int)(at[j] % Wh);
        const double w = (kw > 0 && 2 * kw != W) ? 2.0 : 1.0;
        const double ar = (double)xr[at[j]], ai = (double)xi[at[j]];
        n += w;
        sxx += w * (ar * ar + ai * ai);
        if (yre) {
            const double br = (double)yre[at[j]], bi = (double)yim[at[j]];
            const double dr = ar - br, di = ai - bi;
            syy += w * (br * br + bi * bi);
            sxy += w * (ar * br + ai * bi);
            see += w * (dr * dr + di * di);
        }
    }
    double rec[SpCols::COLS];
    rec[DDPM3D_SP_N] = n;
    rec[DDPM3D_SP_SUM_XX] = sxx;
    rec[DDPM3D_SP_SUM_YY] = syy;
    rec[DDPM3D_SP_SUM_XY] = sxy;
    rec[DDPM3D_SP_SUM_EE] = see;
    rr_write_record<SpCols, SP_THREADS>(rec, ws + ((int64_t)b * total + c) * DDPM3D_SP_REC);
}

// Workgroup (s, b): the shell's records in ascending order; a shell without a chunk gets zeros.
__global__ __launch_bounds__(SP_THREADS) void sp_fold_kernel(const double* __restrict__ ws,
                                                             const int64_t* __restrict__ chunks, int64_t total, int S,
                                                             double* __restrict__ out) {
    const int s = blockIdx.x, b = blockIdx.y;
    const int64_t c0 = chunks[s], c1 = chunks[s + 1];
    rr_fold_record<SpCols, SP_THREADS>(ws + ((int64_t)b * total + c0) * DDPM3D_SP_REC, c1 - c0,
                                       out + ((int64_t)b * S + s) * DDPM3D_SP_REC);
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t planes_bytes(int B, int D, int H, int W) {         // one re and one im plane of B spectra
    return up16((size_t)2 * B * D * H * (W / 2 + 1) * sizeof(float));
}

}  // namespace

size_t ddpm3d_dft_workspace_bytes(int B, int D, int H, int W) { return planes_bytes(B, D, H, W); }

// W pass into (re, im), H pass into the workspace, D pass back into (re, im); `only` in 0..2 runs that pass alone over
// whatever its input buffer holds (timing), -1 all three
hipError_t ddpm3d_launch_dft3(const float* vol, const float* pivot, int B, int D, int H, int W,
                              const ddpm3d_dft_axis* axes, void* ws, float* re, float* im, int only, hipStream_t st) {
    const int Wh = W / 2 + 1;
    const int64_t plane = (int64_t)B * D * H * Wh;
    float* tr = (float*)ws;
    float* ti = tr + plane;
    DftPass p = {};
    if (only < 0 || only == 0) {
        p.cos_t = axes[2].cos_t, p.sin_t = axes[2].sin_t, p.n = W, p.R = Wh;
        p.M = (int64_t)B * D * H, p.N = 2 * Wh, p.K = W;
        p.in_re = vol, p.in_im = nullptr, p.out_re = re, p.out_im = im;
        p.pivot = pivot, p.rows_per_volume = D * H;
        const hipError_t e = launch_pass<true>(p, 1, st);
        if (e != hipSuccess) return e;
    }
    p.pivot = nullptr;
    if (only < 0 || only == 1) {
        p.cos_t = axes[1].cos_t, p.sin_t = axes[1].sin_t, p.n = H, p.R = H;
        p.M = 2 * H, p.N = Wh, p.K = 2 * H;
        p.in_re = re, p.in_im = im, p.out_re = tr, p.out_im = ti;
        const hipError_t e = launch_pass<false>(p, (int64_t)B * D, st);
        if (e != hipSuccess) return e;
    }
    if (only < 0 || only == 2) {
        p.cos_t = axes[0].cos_t, p.sin_t = axes[0].sin_t, p.n = D, p.R = D;
        p.M = 2 * D, p.N = H * Wh, p.K = 2 * D;
        p.in_re = tr, p.in_im = ti, p.out_re = re, p.out_im = im;
        return launch_pass<false>(p, B, st);
    }
    return hipSuccess;
}

size_t ddpm3d_sp_workspace_bytes(int B, int64_t chunks) {
    return up16((size_t)B * (size_t)(chunks > 0 ? chunks : 1) * DDPM3D_SP_REC * sizeof(double));
}

hipError_t ddpm3d_launch_shell_sums(const float* xre, const float* xim, const float* yre, const float* yim, int B,
                                    int D, int H, int W, const ddpm3d_roi_index& ix, int64_t chunks, double* ws,
                                    double* out, hipStream_t st) {
    const int Wh = W / 2 + 1;
    if (chunks > 0) {
        hipLaunchKernelGGL(sp_chunk_kernel, dim3((unsigned)chunks, B), dim3(SP_THREADS), 0, st, xre, xim, yre, yim,
                           (int64_t)D * H * Wh, W, Wh, ix.regions, ix.d_offsets, ix.d_chunks, ix.d_index, chunks, ws);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sp_fold_kernel, dim3(ix.regions, B), dim3(SP_THREADS), 0, st, ws, ix.d_chunks, chunks,
                       ix.regions, out);
    return hipGetLastError();
}

// Workspace: [target re, im] (with a target), [B estimates' re, im], [one volume's pass planes], [shell records].
size_t ddpm3d_spectrum_workspace_bytes(int B, int D, int H, int W, int64_t chunks, int with_target) {
    return (with_target ? planes_bytes(1, D, H, W) : 0) + planes_bytes(B, D, H, W) + planes_bytes(1, D, H, W) +
           ddpm3d_sp_workspace_bytes(B, chunks);
}

hipError_t ddpm3d_launch_shell_spectrum(const float* est, const float* est_pivot, const float* target,
                                        const float* target_pivot, int B, int D, int H, int W,
                                        const ddpm3d_dft_axis* axes, const ddpm3d_roi_index& ix, int64_t chunks,
                                        void* ws, double* out, hipStream_t st) {
    const int64_t coeffs = (int64_t)D * H * (W / 2 + 1);
    char* at = (char*)ws;
    float *yre = nullptr, *yim = nullptr;
    if (target) {
        yre = (float*)at, yim = yre + coeffs;
        at += planes_bytes(1, D, H, W);
    }
    float* xre = (float*)at;
    float* xim = xre + (int64_t)B * coeffs;
    at += planes_bytes(B, D, H, W);
    void* pass = at;
    at += planes_bytes(1, D, H, W);
    if (target) {
        const hipError_t e = ddpm3d_launch_dft3(target, target_pivot, 1, D, H, W, axes, pass, yre, yim, -1, st);
        if (e != hipSuccess) return e;
    }
    // one volume at a time: the pass planes stay those of one volume whatever B is
    for (int b = 0; b < B; ++b) {
        const hipError_t e = ddpm3d_launch_dft3(est + (int64_t)b * D * H * W, est_pivot ? est_pivot + b : nullptr, 1,
                                                D, H, W, axes, pass, xre + b * coeffs, xim + b * coeffs, -1, st);
        if (e != hipSuccess) return e;
    }
    return ddpm3d_launch_shell_sums(xre, xim, yre, yim, B, D, H, W, ix, chunks, (double*)at, out, st);
}
