// Small gfx950 kernels around the conv: weight packing, GroupNorm statistics
// folding, timestep embedding, Linear, layout changes and the per-step
// sampler update.  All HBM- or latency-bound; wave64 throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "conv3d_params.h"
#include "conv3d_load.h"   // affine_act, act_quad, half_pack
#include "ops.h"
#include "noise.h"
#include "record_reduce.h"

// ------------------------------------------------------------------ packing
// OIDHW -> [tap][ci/8][CoutPad][8]  (zero padded in ci and cout).  The inner 8
// is the channel within the 8-block; lane half h of the conv reads [4h, 4h+4).
__global__ void pack_weight_kernel(const float* __restrict__ w, int Cout, int Cin, int taps,
                                   int CoutPad, int CinPad, float* __restrict__ out) {
    const size_t total = (size_t)taps * CinPad * CoutPad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        size_t r = i >> 3;
        const int co = (int)(r % CoutPad); r /= CoutPad;
        const int cb = (int)(r % (CinPad / 8));
        const int tap = (int)(r / (CinPad / 8));
        const int ci = cb * 8 + j;
        float v = 0.0f;
        if (co < Cout && ci < Cin) v = w[((size_t)co * Cin + ci) * taps + tap];
        out[i] = v;
    }
}

// The 16-bit images.  A weight source says how many taps a form has and what tap `tap` of a (cout, ci) pair
// is in fp32; the two kernels below know nothing else about a form.
struct PlainTaps {   // the OIDHW weights themselves (27 taps, or 1)
    int n;
    __device__ int taps() const { return n; }
    __device__ float at(const float* __restrict__ w, size_t co_ci, int tap) const { return w[co_ci * n + tap]; }
};

// Winograd F(2,3) along depth (conv3d_wz.h): weight transform at pack time.  For every
// (cout, ci, dy, dx): U0 = g0, U1 = (g0+g1+g2)/2, U2 = (g0-g1+g2)/2, U3 = g2 with g_k the
// weight at dz = k; 36 "taps" ordered (j, dy, dx).
__device__ __forceinline__ float wz_weight(const float* __restrict__ w, size_t co_ci, int j, int dydx) {
    const float g0 = w[co_ci * 27 + dydx], g1 = w[co_ci * 27 + 9 + dydx], g2 = w[co_ci * 27 + 18 + dydx];
    if (j == 0) return g0;
    if (j == 3) return g2;
    return j == 1 ? 0.5f * ((g0 + g2) + g1) : 0.5f * ((g0 + g2) - g1);
}
struct WzTaps {
    __device__ static constexpr int taps() { return 36; }
    __device__ float at(const float* __restrict__ w, size_t co_ci, int tap) const {
        return wz_weight(w, co_ci, tap / 9, tap % 9);
    }
};

// Phase weights of an IN_UP conv (DDPM3D_HINT_UP_PHASE, conv3d_wz.h PHASE): on the 2x nearest-up-sampled plane
// the taps dy of an output row of parity py meet two source rows -- py = 0: {0} | {1, 2}, py = 1: {0, 1} | {2} --
// and the same along x.  Phase tap t = j*4 + a*2 + b of phase ph = 2 py + px is the fp32 sum of the shipped
// U_j[dy][dx] (wz_weight) over group a of py x group b of px, added in (dy, dx) row-major order.
__device__ __forceinline__ float wz_up_weight(const float* __restrict__ w, size_t co_ci, int ph, int t) {
    const int py = ph >> 1, px = ph & 1, j = t >> 2, a = (t >> 1) & 1, b = t & 1;
    const int dy0 = a ? 1 + py : 0, dy1 = a ? 2 : py;
    const int dx0 = b ? 1 + px : 0, dx1 = b ? 2 : px;
    float s = 0.0f;
    bool first = true;
    for (int dy = dy0; dy <= dy1; ++dy)
        for (int dx = dx0; dx <= dx1; ++dx) {
            const float u = wz_weight(w, co_ci, j, dy * 3 + dx);
            s = first ? u : s + u;
            first = false;
        }
    return s;
}
struct WzUpTaps {   // 64 "taps": phase * 16 + phase tap
    __device__ static constexpr int taps() { return 64; }
    __device__ float at(const float* __restrict__ w, size_t co_ci, int tap) const {
        return wz_up_weight(w, co_ci, tap >> 4, tap & 15);
    }
};

// Pass 1: per output channel, over all of the form's taps, the power-of-two scale
// s = 2^floor(log2(W_TARGET / max|w|)) and the epilogue factor 1 / s.  unit (the bf16 images, which are not
// scaled): 1 without reading w.
template <class Src>
__global__ __launch_bounds__(256) void pack_scale_kernel(Src src, const float* __restrict__ w, int Cout, int Cin,
                                                         bool unit, float* __restrict__ wscale) {
    const int co = blockIdx.x;
    float m = 0.0f;
    if (co < Cout && !unit)
        for (int i = threadIdx.x; i < Cin * src.taps(); i += 256)
            m = fmaxf(m, fabsf(src.at(w, (size_t)co * Cin + i / src.taps(), i % src.taps())));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float s = 1.0f;
        if (m > 0.0f && m < 3.0e38f) s = exp2f(floorf(log2f(DDPM3D_X3_W_TARGET / m)));
        s = fminf(fmaxf(s, 1.0f / 16777216.0f), 16777216.0f);
        wscale[co] = 1.0f / s;  // exact: powers of two
    }
}

// Pass 2: -> [tap][ci/16][hi|lo][CoutPad][16 f16] of w * s[cout] (zero padded),
// with s = 1 / wscale[cout] recovered exactly from pass 1's output.
// bf16 = true: the bf16 mode's image in the same layout -- hi = bf16(w) (no scale, wscale = 1), lo = 0
__device__ __forceinline__ _Float16 bf16_bits_as_h(float v) {
    return __builtin_bit_cast(_Float16, __builtin_bit_cast(unsigned short, (__bf16)v));
}
template <class Src>
__global__ void pack_split_kernel(Src src, const float* __restrict__ w, const float* __restrict__ wscale, int Cout,
                                  int Cin, int CoutPad, int CinPad, _Float16* __restrict__ out, bool bf16) {
    const size_t total = (size_t)src.taps() * CinPad * CoutPad;  // one (hi, lo) pair per element
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 15);
        size_t r = i >> 4;
        const int co = (int)(r % CoutPad); r /= CoutPad;
        const int cb = (int)(r % (CinPad / 16));
        const int tap = (int)(r / (CinPad / 16));
        const int ci = cb * 16 + j;
        float v = 0.0f;
        if (co < Cout && ci < Cin) v = src.at(w, (size_t)co * Cin + ci, tap) * (1.0f / wscale[co]);
        const _Float16 hi = bf16 ? bf16_bits_as_h(v) : (_Float16)v;
        const _Float16 lo = bf16 ? (_Float16)0.0f : (_Float16)(v - (float)hi);
        const size_t base = (((size_t)tap * (CinPad / 16) + cb) * 2) * CoutPad * 16;
        out[base + (size_t)co * 16 + j] = hi;
        out[base + (size_t)CoutPad * 16 + (size_t)co * 16 + j] = lo;
    }
}

static int pack_blocks(const PackedImage& img) {   // one thread per 4-byte element, grid-stride beyond 4096 blocks
    const size_t blocks = (img.body / 4 + 255) / 256;
    return blocks > 4096 ? 4096 : (int)blocks;
}

// one 16-bit image at `out`: the scales behind the taps first, then the taps
template <class Src>
static hipError_t launch_pack16(Src src, const PackedImage& img, const float* w, int Cout, int Cin, bool bf16,
                                void* out, hipStream_t st) {
    const int CoutPad = ddpm3d_cout_pad(Cout), CinPad = ddpm3d_cin_pad(Cin);
    float* wscale = reinterpret_cast<float*>(reinterpret_cast<char*>(out) + img.body);
    hipLaunchKernelGGL(pack_scale_kernel<Src>, dim3(CoutPad), dim3(256), 0, st, src, w, Cout, Cin, bf16, wscale);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pack_split_kernel<Src>, dim3(pack_blocks(img)), dim3(256), 0, st, src, w, wscale, Cout, Cin,
                       CoutPad, CinPad, (_Float16*)out, bf16);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_pack_up_phase(const float* w, int Cout, int Cin, void* out, hipStream_t st) {
    // the shipped Winograd-D image in front (the shapes that fall back run on it), the phase image behind it
    hipError_t e = ddpm3d_launch_pack(w, Cout, Cin, 3, DDPM3D_PREC_F16X3_WZ, out, st);
    if (e != hipSuccess) return e;
    char* body = reinterpret_cast<char*>(out) + ddpm3d_packed_image(Cout, Cin, 3, DDPM3D_PREC_F16X3_WZ).bytes();
    return launch_pack16(WzUpTaps{}, ddpm3d_up_phase_image(Cout, Cin), w, Cout, Cin, false, body, st);
}

hipError_t ddpm3d_launch_pack(const float* w, int Cout, int Cin, int ks, int prec, void* out, hipStream_t st) {
    const PackedImage img = ddpm3d_packed_image(Cout, Cin, ks, prec);
    if (prec == DDPM3D_PREC_F32) {
        hipLaunchKernelGGL(pack_weight_kernel, dim3(pack_blocks(img)), dim3(256), 0, st, w, Cout, Cin, img.taps,
                           ddpm3d_cout_pad(Cout), ddpm3d_cin_pad(Cin), (float*)out);
        return hipGetLastError();
    }
    const bool bf16 = ddpm3d_prec_bf16(prec);
    if (ddpm3d_prec_wz(prec)) return launch_pack16(WzTaps{}, img, w, Cout, Cin, bf16, out, st);
    return launch_pack16(PlainTaps{img.taps}, img, w, Cout, Cin, bf16, out, st);
}

// ------------------------------------------------------------- wave helpers
// (wave_sum(double) is record_reduce.h's)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------- GN finalize
// One workgroup per (n, group): fold partial (sum, sumsq) rows in fp64, then
// write A, B for the group's channels.  256 threads, or 1024 where a group's run of partial sums
// is long (the launcher decides from the shape alone, so results stay repeatable): the kernel is a
// latency chain -- N x 32 workgroups on 256 CUs, each waiting for its own loads -- and four times
// the loads in flight cut the long ones (2048 rows at the 64^3 level: 128 KB per group) from
// 17-33 us to the launch floor (r03: the fp64 statistics had doubled this kernel's bytes).
__global__ __launch_bounds__(1024) void gn_finalize_kernel(
    const double* __restrict__ st0, int C0, int rows0, const double* __restrict__ st1, int C1, int rows1,
    int groups, double count, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ film, int film_stride, int film_off, float* __restrict__ A,
    float* __restrict__ B, float* __restrict__ bound) {
    const int C = C0 + C1;
    const int cg = C / groups;
    const int n = blockIdx.x / groups, g = blockIdx.x % groups;
    const int cbeg = g * cg;
    const bool from0 = cbeg < C0;
    const double* st = from0 ? st0 : st1;
    const int Cs = from0 ? C0 : C1;
    const int rows = from0 ? rows0 : rows1;
    const int cs = from0 ? cbeg : cbeg - C0;
    // statistics are channel-major [N][C][rows][2] fp64: the group's cg channels x rows partial sums
    // are ONE contiguous, 16-byte aligned run of cg*rows (sum, sum of squares) pairs
    // the affine's inputs do not depend on the statistics: requested FIRST, so that their latency runs
    // beside the partial-sum loads' instead of behind the reduction (one dependent round trip less)
    const int c_own = cbeg + (int)(threadIdx.x < (unsigned)cg ? threadIdx.x : 0);
    float g_own = 0.0f, b_own = 0.0f, sc_own = 1.0f, sh_own = 0.0f;
    if (gamma != nullptr) {
        g_own = gamma[c_own];
        b_own = beta[c_own];
        if (film != nullptr) {
            sc_own = 1.0f + film[(size_t)n * film_stride + film_off + c_own];
            sh_own = film[(size_t)n * film_stride + film_off + C + c_own];
        }
    }
    double s1 = 0.0, s2 = 0.0;
    float m2 = 0.0f;                                  // largest sum of squares of any row of the group
    const size_t items = (size_t)rows * cg;          // double2 count
    const double2* run = reinterpret_cast<const double2*>(st + ((size_t)n * Cs + cs) * rows * 2);
    // Eight 16-byte loads in flight per thread, UNCONDITIONALLY: buffer loads past the run return zeros, which change
    // neither sum nor maximum.  (r01-r04 had `#pragma unroll 8` on a loop with a run-time trip count: what came out
    // was eight guarded loads, each behind an s_waitcnt vmcnt(0) -- eight dependent round trips for the 64^3 level's
    // eight items per thread, 12-15 us of the kernel's 5 us floor.  Same additions in the same order.)
    {
        const unsigned bytes = items * 16 < 0xFFFFFFF0ull ? (unsigned)(items * 16) : 0xFFFFFFF0u;
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(run, bytes);
        const unsigned step = blockDim.x * 16u;
        for (size_t i0 = 0; i0 < items; i0 += (size_t)blockDim.x * 8) {
            u32x4 t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = buffer_load16(rr, (unsigned)(i0 + threadIdx.x) * 16u + k * step, 0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double2 v = __builtin_bit_cast(double2, t[k]);
                s1 += v.x;
                s2 += v.y;
                m2 = fmaxf(m2, (float)v.y);
            }
        }
    }
    __shared__ double red[2][16];
    __shared__ float redm[16], redab[2][16];
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m2 = fmaxf(m2, __shfl_xor(m2, o));
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = s1; red[1][wave] = s2; redm[wave] = m2; }
    __syncthreads();
    s1 = 0.0; s2 = 0.0; m2 = 0.0f;
    for (int w = 0; w < nwaves; ++w) {               // fixed order: the same sums on every run
        s1 += red[0][w];
        s2 += red[1][w];
        m2 = fmaxf(m2, redm[w]);
    }
    // every |x| of the group is at most the square root of the largest row's sum of squares -- of its EXACT sum of
    // squares: the conv epilogues' pivoted fp32 sums can leave it short by the relative slack delta of ddpm3d.h
    const float xmax = sqrtf(m2);
    if (gamma == nullptr) {                          // bounds only (tensor consumed without a GroupNorm)
        if (threadIdx.x == 0 && bound != nullptr) {
            bound[(size_t)blockIdx.x * 2] = xmax;
            bound[(size_t)blockIdx.x * 2 + 1] = xmax;
        }
        return;
    }
    const double cnt = count * cg;
    const double mean = s1 / cnt;
    double var = s2 / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float meanf = (float)mean;
    float amax = 0.0f, bmax = 0.0f;
    for (int c = threadIdx.x; c < cg; c += blockDim.x) {
        const int ch = cbeg + c;
        const bool own = c == (int)threadIdx.x;       // (cg <= blockDim.x: every channel is some thread's own)
        float a = rstd * (own ? g_own : gamma[ch]);
        float b = fmaf(-meanf, a, own ? b_own : beta[ch]);
        if (film != nullptr) {
            const float sc = own ? sc_own : 1.0f + film[(size_t)n * film_stride + film_off + ch];
            const float sh = own ? sh_own : film[(size_t)n * film_stride + film_off + C + ch];
            a = a * sc;
            b = fmaf(b, sc, sh);
        }
        A[(size_t)n * C + ch] = a;
        B[(size_t)n * C + ch] = b;
        amax = fmaxf(amax, fabsf(a));
        bmax = fmaxf(bmax, fabsf(b));
    }
    if (bound != nullptr) {
        // |act(a x + b)| <= |a| xmax + |b| for act = identity or SiLU
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            amax = fmaxf(amax, __shfl_xor(amax, o));
            bmax = fmaxf(bmax, __shfl_xor(bmax, o));
        }
        if ((threadIdx.x & 63) == 0) { redab[0][wave] = amax; redab[1][wave] = bmax; }
        __syncthreads();
        if (threadIdx.x == 0) {
            amax = 0.0f; bmax = 0.0f;
            for (int w = 0; w < nwaves; ++w) {
                amax = fmaxf(amax, redab[0][w]);
                bmax = fmaxf(bmax, redab[1][w]);
            }
            bound[(size_t)blockIdx.x * 2] = fmaf(amax, xmax, bmax);
            bound[(size_t)blockIdx.x * 2 + 1] = xmax;
        }
    }
}

// max |x| per sample of up to two tensors: bound[n * count + t].  ABSMAX_PARTS workgroups per (sample, tensor)
// fold their slices with an atomic max on the bit patterns (non-negative floats order like unsigned integers:
// exact, so the result does not depend on arrival order); the launcher zeroes `bound` first.  (r03: ONE
// 1024-thread workgroup per tensor walked its 1 MB in a 64-deep dependent loop: 36 us per DDPM step.)
#define ABSMAX_PARTS 32
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                     size_t per_sample, int count, float* __restrict__ bound) {
    const int part = blockIdx.x % ABSMAX_PARTS, nt = blockIdx.x / ABSMAX_PARTS;
    const int n = nt / count, t = nt % count;
    const float* x = (t == 0 ? x0 : x1) + (size_t)n * per_sample;
    float m = 0.0f;
    const size_t quads = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? per_sample / 4 : 0;
    const size_t qper = (quads + ABSMAX_PARTS - 1) / ABSMAX_PARTS;
    const size_t q0 = (size_t)part * qper, q1 = q0 + qper < quads ? q0 + qper : quads;
#pragma unroll 4
    for (size_t i = q0 + threadIdx.x; i < q1; i += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + i * 4);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    if (part == 0)   // the unaligned / remainder elements
        for (size_t i = quads * 4 + threadIdx.x; i < per_sample; i += 256) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = fmaxf(m, red[w]);
        // m is a non-negative, non-NaN float (fmaxf drops NaNs): its bits order like the value
        atomicMax(reinterpret_cast<unsigned*>(bound) + nt, __float_as_uint(m));
    }
}

hipError_t ddpm3d_launch_absmax(const float* x0, const float* x1, int N, size_t per_sample, float* bound,
                                hipStream_t st) {
    const int count = x1 ? 2 : 1;
    hipError_t e = hipMemsetAsync(bound, 0, sizeof(float) * (size_t)N * count, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(absmax_kernel, dim3(N * count * ABSMAX_PARTS), dim3(256), 0, st, x0, x1, per_sample, count, bound);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_gn_finalize(const double* st0, int C0, int rows0, const double* st1, int C1,
                                     int rows1, int N, int groups, double count, float eps,
                                     const float* gamma, const float* beta, const float* film,
                                     int film_stride, int film_off, float* A, float* B, float* bound,
                                     hipStream_t st) {
    const long long items = (long long)(rows0 > rows1 ? rows0 : rows1) * ((C0 + C1) / groups);   // double2 per group
    const int threads = items >= 2048 ? 1024 : 256;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(N * groups), dim3(threads), 0, st, st0, C0, rows0, st1, C1,
                       rows1, groups, count, eps, gamma, beta, film, film_stride, film_off, A, B, bound);
    return hipGetLastError();
}

// --------------------------------------------------------------- GN stats
// Stand-alone statistics pass for NDHWC tensors no conv epilogue produced.
// One workgroup per (n, row of GN_STATS_VOX voxels): thread c-strided over
// channels, 16-byte loads along C.
#define GN_STATS_VOX 256
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, int voxels, int C,
                                                       int rows, double* __restrict__ stats) {
    const int n = blockIdx.x / rows, r = blockIdx.x % rows;
    const int v0 = r * GN_STATS_VOX;
    const int v1 = min(v0 + GN_STATS_VOX, voxels);
    const int C4 = C / 4;
    // thread -> (channel quad, voxel lane); quads fastest so a wave reads contiguous bytes
    const int qpt = min(C4, 256);
    const int vlanes = 256 / qpt;
    __shared__ double sh[2][256 * 4];
    for (int q0 = 0; q0 < C4; q0 += qpt) {
        const int q = q0 + (threadIdx.x % qpt);
        const int vl = threadIdx.x / qpt;
        double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};   // fp64 sums (cf. conv3d_params.h: GnAcc, the conv epilogues' pivoted fp32 form)
        if (q < C4 && vl < vlanes) {
            for (int v = v0 + vl; v < v1; v += vlanes) {
                const float4 t = *reinterpret_cast<const float4*>(x + ((size_t)n * voxels + v) * C + q * 4);
                const double tx = t.x, ty = t.y, tz = t.z, tw = t.w;
                s1[0] += tx; s1[1] += ty; s1[2] += tz; s1[3] += tw;
                s2[0] = fma(tx, tx, s2[0]); s2[1] = fma(ty, ty, s2[1]);
                s2[2] = fma(tz, tz, s2[2]); s2[3] = fma(tw, tw, s2[3]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { sh[0][threadIdx.x * 4 + i] = s1[i]; sh[1][threadIdx.x * 4 + i] = s2[i]; }
        __syncthreads();
        if (threadIdx.x < qpt && q < C4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double a = 0.0, b = 0.0;
                for (int l = 0; l < vlanes; ++l) {
                    a += sh[0][(l * qpt + threadIdx.x) * 4 + i];
                    b += sh[1][(l * qpt + threadIdx.x) * 4 + i];
                }
                double* o = stats + (((size_t)n * C + q * 4 + i) * rows + r) * 2;
                o[0] = a;
                o[1] = b;
            }
        }
        __syncthreads();
    }
}

hipError_t ddpm3d_launch_gn_stats(const float* x, int N, int voxels, int C, double* stats, hipStream_t st) {
    const int rows = (voxels + GN_STATS_VOX - 1) / GN_STATS_VOX;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(N * rows), dim3(256), 0, st, x, voxels, C, rows, stats);
    return hipGetLastError();
}
int ddpm3d_gn_stats_rows_impl(int voxels) { return (voxels + GN_STATS_VOX - 1) / GN_STATS_VOX; }

// ------------------------------------------------------ timestep embedding
__global__ void timestep_embedding_kernel(const float* __restrict__ t, int rows, int dim,
                                          const float* __restrict__ freqs, float* __restrict__ out) {
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * dim) return;
    const int r = i / dim, j = i - r * dim;
    float v = 0.0f;
    if (j < 2 * half) {
        const int f = j < half ? j : j - half;
        // args = t * freqs in fp32 (nn.py:116); cos / sin evaluated in fp64 and rounded
        // once, i.e. the correctly rounded fp32 value a <=1-ulp fp32 libm returns almost always
        const float arg = t[r] * freqs[f];
        v = j < half ? (float)cos((double)arg) : (float)sin((double)arg);
    }
    out[i] = v;
}

hipError_t ddpm3d_launch_timestep_embedding(const float* t, int rows, int dim, const float* freqs,
                                            float* out, hipStream_t st) {
    const int total = rows * dim;
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((total + 255) / 256), dim3(256), 0, st, t, rows, dim,
                       freqs, out);
    return hipGetLastError();
}

// ------------------------------------------------- pooled activation (pre-pass)
// out[n][z][y][x][c] = mean over the (1,2,2) window of act(A[n][c] * src + B[n][c]): the IN_POOL prologue of
// ddpm3d_conv3d (conv3d_load.h halo_fetch: same window order, same SiLU) as a pass of its own, so that the
// down ResBlocks' first conv (unet.py:238-242: h = in_conv(h_upd(in_rest(x)))) can run the Winograd-D form on
// a plain tensor.  One thread = one output voxel x 4 channels: four 16-byte loads, one 16-byte store.
template <bool FAST>
__global__ __launch_bounds__(256) void pool_act_kernel(const float* __restrict__ src, const float* __restrict__ A,
                                                       const float* __restrict__ B, int act, int N, int D, int H,
                                                       int W, int C, float* __restrict__ out, int src16,
                                                       int out16, int f16) {
    const int quads = C >> 2;
    const size_t total = (size_t)N * D * H * W * quads;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int cq = (int)(i % quads);
    size_t v = i / quads;
    const int x = (int)(v % W); v /= W;
    const int y = (int)(v % H); v /= H;
    const int z = (int)(v % D);
    const int n = (int)(v / D);
    const size_t Ws = 2 * (size_t)W, Hs = 2 * (size_t)H;
    const size_t e0 = ((((size_t)n * D + z) * Hs + 2 * y) * Ws + 2 * x) * C + cq * 4;
    f32x4 s00 = act_quad(src, e0, src16 != 0, f16 != 0);
    f32x4 s01 = act_quad(src, e0 + C, src16 != 0, f16 != 0);
    f32x4 s10 = act_quad(src, e0 + Ws * C, src16 != 0, f16 != 0);
    f32x4 s11 = act_quad(src, e0 + Ws * C + C, src16 != 0, f16 != 0);
    if (A != nullptr) {
        const f32x4 ga = *reinterpret_cast<const f32x4*>(A + (size_t)n * C + cq * 4);
        const f32x4 gb = *reinterpret_cast<const f32x4*>(B + (size_t)n * C + cq * 4);
        if (act) {
            s00 = affine_act<1, FAST>(s00, ga, gb); s01 = affine_act<1, FAST>(s01, ga, gb);
            s10 = affine_act<1, FAST>(s10, ga, gb); s11 = affine_act<1, FAST>(s11, ga, gb);
        } else {
            s00 = affine_act<0, FAST>(s00, ga, gb); s01 = affine_act<0, FAST>(s01, ga, gb);
            s10 = affine_act<0, FAST>(s10, ga, gb); s11 = affine_act<0, FAST>(s11, ga, gb);
        }
    }
    // AvgPool3d window order (h, w): ((s00 + s01) + s10) + s11, then * 1/4
    const f32x4 r = (((s00 + s01) + s10) + s11) * 0.25f;
    const size_t eo = i * 4;
    if (out16)
        *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(out) + eo) =
            u32x2{half_pack(r[0], r[1], f16 != 0), half_pack(r[2], r[3], f16 != 0)};
    else
        *reinterpret_cast<f32x4*>(out + eo) = r;
}

hipError_t ddpm3d_launch_pool_act(const float* src, const float* A, const float* B, int act, int fast, int N, int D,
                                  int H, int W, int C, float* out, int src16, int out16, int f16, hipStream_t st) {
    const size_t total = (size_t)N * D * H * W * (C / 4);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (fast)
        hipLaunchKernelGGL(pool_act_kernel<true>, dim3(blocks), dim3(256), 0, st, src, A, B, act, N, D, H, W, C, out,
                           src16, out16, f16);
    else
        hipLaunchKernelGGL(pool_act_kernel<false>, dim3(blocks), dim3(256), 0, st, src, A, B, act, N, D, H, W, C, out,
                           src16, out16, f16);
    return hipGetLastError();
}

// ------------------------------------------------------------ label embedding
// emb[r][:] += table[idx[r]][:]  (unet.py:703-705: emb = emb + self.label_emb(y))
// A label outside [0, num_classes) reads nothing (its row stays as it was): the C ABI is safe by itself,
// the Python host still refuses such labels where nn.Embedding would.
__global__ void add_embedding_kernel(float* __restrict__ emb, const float* __restrict__ table,
                                     const int64_t* __restrict__ idx, int rows, int dim, int num_classes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * dim) return;
    const int r = i / dim, j = i - r * dim;
    const int64_t c = idx[r];
    if ((uint64_t)c < (uint64_t)num_classes) emb[i] += table[(size_t)c * dim + j];
}

hipError_t ddpm3d_launch_add_embedding(float* emb, const float* table, const int64_t* idx, int rows, int dim,
                                       int num_classes, hipStream_t st) {
    const int total = rows * dim;
    hipLaunchKernelGGL(add_embedding_kernel, dim3((total + 255) / 256), dim3(256), 0, st, emb, table, idx, rows, dim,
                       num_classes);
    return hipGetLastError();
}

// ------------------------------------------------------------------ linear
// One wave per output feature o, LIN_ROWS rows of the batch at a time: the
// weight row is read once (coalesced 256-B segments) and reused across rows.
#define LIN_ROWS 8
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ in, int rows, int K,
                                                     const float* __restrict__ w,
                                                     const float* __restrict__ bias, int O, int silu_in,
                                                     float* __restrict__ out, int out_stride) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r0 = blockIdx.y * LIN_ROWS;
    if (o >= O) return;
    float acc[LIN_ROWS];
#pragma unroll
    for (int r = 0; r < LIN_ROWS; ++r) acc[r] = 0.0f;
    for (int k = lane; k < K; k += 64) {
        const float wv = w[(size_t)o * K + k];
#pragma unroll
        for (int r = 0; r < LIN_ROWS; ++r) {
            if (r0 + r < rows) {
                float xv = in[(size_t)(r0 + r) * K + k];
                if (silu_in) xv = xv / (1.0f + expf(-xv));
                acc[r] = fmaf(xv, wv, acc[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < LIN_ROWS; ++r) {
        const float s = wave_sum(acc[r]);
        if (lane == 0 && r0 + r < rows) out[(size_t)(r0 + r) * out_stride + o] = s + bias[o];
    }
}

hipError_t ddpm3d_launch_linear(const float* in, int rows, int K, const float* w, const float* bias, int O,
                                int silu_in, float* out, int out_stride, hipStream_t st) {
    dim3 grid((O + 3) / 4, (rows + LIN_ROWS - 1) / LIN_ROWS);
    hipLaunchKernelGGL(linear_kernel, grid, dim3(256), 0, st, in, rows, K, w, bias, O, silu_in, out,
                       out_stride);
    return hipGetLastError();
}

// ----------------------------------------------------------------- layouts
// LDS-tiled transpose between [C][V] and [V][C] per sample (32x32 tiles, +1 pad).
__global__ __launch_bounds__(256) void transpose_cv_kernel(const float* __restrict__ in, int R, int S,
                                                           float* __restrict__ out) {
    // in: [n][R][S] -> out: [n][S][R]
    __shared__ float tile[32][33];
    const int n = blockIdx.z;
    const int s0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const float* src = in + (size_t)n * R * S;
    float* dst = out + (size_t)n * R * S;
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int r = r0 + ty + j, s = s0 + tx;
        tile[ty + j][tx] = (r < R && s < S) ? src[(size_t)r * S + s] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int s = s0 + ty + j, r = r0 + tx;
        if (r < R && s < S) dst[(size_t)s * R + r] = tile[tx][ty + j];
    }
}

__global__ __launch_bounds__(256) void to_ndhwc_pad_kernel(const float* __restrict__ in, int C, int voxels, int Cpad,
                                                           float* __restrict__ out) {
    const int n = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= voxels) return;
    float* o = out + ((size_t)n * voxels + v) * Cpad;
    for (int c = 0; c < Cpad; ++c) o[c] = c < C ? in[((size_t)n * C + c) * voxels + v] : 0.0f;
}
hipError_t ddpm3d_launch_to_ndhwc_pad(const float* in, int N, int C, int voxels, int Cpad, float* out, hipStream_t st) {
    hipLaunchKernelGGL(to_ndhwc_pad_kernel, dim3((voxels + 255) / 256, N), dim3(256), 0, st, in, C, voxels, Cpad, out);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_transpose(const float* in, int N, int R, int S, float* out, hipStream_t st) {
    dim3 grid((S + 31) / 32, (R + 31) / 32, N);
    hipLaunchKernelGGL(transpose_cv_kernel, grid, dim3(256), 0, st, in, R, S, out);
    return hipGetLastError();
}

// out[n][z][y][x][:] = in[n][z][2y][2x][:]  (NDHWC, C % 4 == 0): the even positions of a
// stride-1 conv output = the stride-(1,2,2) conv of Downsample(use_conv=True), unet.py:129-133.
__global__ __launch_bounds__(256) void subsample_hw2_kernel(const float4* __restrict__ in, int D, int H, int W,
                                                            int C4, float4* __restrict__ out, size_t total) {
    const int Ho = H / 2, Wo = W / 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4);
        size_t v = i / C4;
        const int x = (int)(v % Wo); v /= Wo;
        const int y = (int)(v % Ho); v /= Ho;   // v = n * D + z
        out[i] = in[((v * H + 2 * y) * W + 2 * x) * C4 + c];
    }
}

hipError_t ddpm3d_launch_subsample_hw2(const float* in, int N, int D, int H, int W, int C, float* out,
                                       hipStream_t st) {
    const size_t total = (size_t)N * D * (H / 2) * (W / 2) * (C / 4);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(subsample_hw2_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(in), D, H, W, C / 4, reinterpret_cast<float4*>(out), total);
    return hipGetLastError();
}

// ---------------------------------------------------------- sampler update
// The arithmetic order mirrors the reference's torch expressions one rounding
// at a time, so contraction into FMAs is switched off here.  The step kernels
// below share the helpers that follow, so every step derives x0, eps and the
// learned variance the same way.
#pragma clang fp contract(off)

// x.clamp(-1, 1): a NaN stays NaN, as in torch (fminf / fmaxf would return the bound for it, and a diverged network's
// output would leave the step as a finite volume); every other input gives the value fminf(fmaxf(x, -1), 1) gives
__device__ __forceinline__ float clamp_unit(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }
// x.clamp(min=lo), NaN kept likewise
__device__ __forceinline__ float clamp_min(float x, float lo) { return x < lo ? lo : x; }

// x0 from the model output's first half (x_start itself, or eps), then the clip
__device__ __forceinline__ float step_x0(float xv, float e, float c_recip, float c_recipm1, int flags) {
    float x0 = (flags & DDPM3D_F_PREDICT_XSTART) ? e : c_recip * xv - c_recipm1 * e;   // :305-311, :328-333
    if (flags & DDPM3D_F_CLIP) x0 = clamp_unit(x0);                                    // :296-297
    return x0;
}

// X0 selects a step kernel's x0 source: the model output's first half (step_x0), or a finished x0 the caller passes
// (the *_step_x0 entries: xs, e.g. ddpm3d_xstart_pull's output), clipped once more under F_CLIP -- the clip is idempotent
template <bool X0>
__device__ __forceinline__ float step_x0_from(const float* __restrict__ mo, const float* __restrict__ xs, size_t i,
                                              size_t first_half, float xv, float c_recip, float c_recipm1, int flags) {
    if (X0) return step_x0(xv, xs[i], c_recip, c_recipm1, flags | DDPM3D_F_PREDICT_XSTART);
    return step_x0(xv, mo[first_half], c_recip, c_recipm1, flags);
}

// LEARNED_RANGE: the model's second half vv in [-1, 1] between the two log-variances
__device__ __forceinline__ float learned_logvar(float vv, float min_log, float max_log) {
    const float frac = (vv + 1.0f) / 2.0f;                      // :274
    return frac * max_log + (1.0f - frac) * min_log;            // :275
}

// _predict_eps_from_xstart
__device__ __forceinline__ float eps_from_x0(float xv, float x0, float c_recip, float c_recipm1) {
    return (c_recip * xv - x0) / c_recipm1;                     // :345-349
}

// The kernels that take T (p_mean_variance, ddim_reverse_step, dpm_solver_step, q_sample, vb_terms) bound t
// themselves: a sample whose t lies outside [0, T) reads no table row and gets NaN in every per-voxel output, a and
// b, b only when has_b, then c and d only when has_cd.  sample_step_kernel takes no T and reads row t_idx[n] as it
// stands: t in [0, rows of coef) is its caller's duty (include/ddpm3d.h), and there this fill serves only a keyed
// patch that leaves its canvas.
__device__ __forceinline__ void step_nan_fill(int n, int voxels, int stride, float* a, float* b, bool has_b, float* c,
                                              float* d, bool has_cd) {
    const float nan = __builtin_nanf("");
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += stride) {
        const size_t i = (size_t)n * voxels + v;
        a[i] = nan;
        if (has_b) b[i] = nan;
        if (has_cd) { c[i] = nan; d[i] = nan; }
    }
}

// element-wise step launches: one grid row per sample, at most 1024 workgroups striding over its voxels
static dim3 step_grid(int N, int voxels) {
    int bx = (voxels + 255) / 256;
    if (bx > 1024) bx = 1024;
    return dim3(bx, N);
}

// Noise: where the step's normal comes from (noise.h) -- the caller's tensor, or the keyed function.  A keyed sample
// whose patch leaves the canvas gets step_nan_fill.
template <bool DDIM, class Noise, bool X0 = false>
__global__ __launch_bounds__(256) void sample_step_kernel(
    const float* __restrict__ mo, const float* __restrict__ xs, const float* __restrict__ x, const Noise noise,
    const float* __restrict__ coef, const int64_t* __restrict__ t_idx, int voxels, int flags, float eta,
    float* __restrict__ sample, float* __restrict__ pred_xstart) {
    const int n = blockIdx.y;
    const int64_t ti = t_idx[n];
    const auto z = noise.sample(n);
    if (!z.ok()) {
        step_nan_fill(n, voxels, gridDim.x * blockDim.x, sample, pred_xstart, pred_xstart != nullptr, nullptr, nullptr,
                      false);
        return;
    }
    const float* c = coef + (size_t)ti * DDPM3D_NCOEF;
    const float c_recip = c[DDPM3D_C_SQRT_RECIP_ACP], c_recipm1 = c[DDPM3D_C_SQRT_RECIPM1_ACP];
    const float c1 = c[DDPM3D_C_POST_MEAN_COEF1], c2 = c[DDPM3D_C_POST_MEAN_COEF2];
    const float min_log = c[DDPM3D_C_MIN_LOG], max_log = c[DDPM3D_C_MAX_LOG];
    const float ab = c[DDPM3D_C_ACP], ab_prev = c[DDPM3D_C_ACP_PREV];
    const bool learn = flags & DDPM3D_F_LEARN_SIGMA;
    const int ch = learn ? 2 : 1;
    const float mask = ti != 0 ? 1.0f : 0.0f;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += gridDim.x * blockDim.x) {
        const size_t i = (size_t)n * voxels + v;
        const float xv = x[i];
        const float x0 = step_x0_from<X0>(mo, xs, i, ((size_t)n * ch) * voxels + v, xv, c_recip, c_recipm1, flags);
        float out;
        if (!DDIM) {
            const float logvar = learn ? learned_logvar(mo[((size_t)n * ch + 1) * voxels + v], min_log, max_log)
                                       : min_log;
            const float mean = c1 * x0 + c2 * xv;                           // :216-219
            out = mean + mask * expf(0.5f * logvar) * z.at(i, v);             // :438
        } else {
            const float eps = eps_from_x0(xv, x0, c_recip, c_recipm1);
            const float sigma = eta * sqrtf((1.0f - ab_prev) / (1.0f - ab)) * sqrtf(1.0f - ab / ab_prev);
            const float mean_pred = x0 * sqrtf(ab_prev) + sqrtf(1.0f - ab_prev - sigma * sigma) * eps;
            out = mean_pred + mask * sigma * z.at(i, v);                     // :584
        }
        sample[i] = out;
        if (pred_xstart != nullptr) pred_xstart[i] = x0;
    }
}

// The run-time-to-template mapping of the step launches, written once: launch(z, t...) gets the step's noise source
// (a KeyNoise where a key is given, else a TensorNoise) and one std::true_type / std::false_type per run-time switch,
// in the order given.
template <class F>
static void with_switches(F&& f) { f(); }
template <class F, class... Rest>
static void with_switches(F&& f, bool on, Rest... rest) {
    if (on) with_switches([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else with_switches([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}
template <class F, class... Switches>
static hipError_t launch_step(const float* noise, const ddpm3d_noise_key* key, F&& launch, Switches... switches) {
    if (key != nullptr) with_switches([&](auto... t) { launch(KeyNoise{noise_key_dev(*key)}, t...); }, switches...);
    else with_switches([&](auto... t) { launch(TensorNoise{noise}, t...); }, switches...);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_sample_step(bool ddim, const float* mo, const float* xs, const float* x, const float* noise,
                                     const ddpm3d_noise_key* key, const float* coef, const int64_t* t_idx, int N,
                                     int voxels, int flags, float eta, float* sample, float* pred_xstart,
                                     hipStream_t st) {
    return launch_step(noise, key, [&](auto z, auto is_ddim, auto has_x0) {
        hipLaunchKernelGGL((sample_step_kernel<is_ddim.value, decltype(z), has_x0.value>), step_grid(N, voxels),
                           dim3(256), 0, st, mo, xs, x, z, coef, t_idx, voxels, flags, eta, sample, pred_xstart);
    }, ddim, xs != nullptr);
}

// ------------------------------------------------- p_mean_variance, DDIM inversion
// The reference's public per-step call (gaussian_diffusion.py:232-326) and the reverse ODE step built on it
// (:587-623), on the step helpers above.

__global__ __launch_bounds__(256) void p_mean_variance_kernel(
    const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ coef,
    const int64_t* __restrict__ t_idx, int voxels, int T, int flags, float* __restrict__ mean,
    float* __restrict__ variance, float* __restrict__ log_variance, float* __restrict__ pred_xstart) {
    const int n = blockIdx.y;
    const int64_t ti = t_idx[n];
    const bool learn = flags & DDPM3D_F_LEARN_SIGMA;
    const int ch = learn ? 2 : 1;
    const int stride = gridDim.x * blockDim.x;
    if (ti < 0 || ti >= T) {
        step_nan_fill(n, voxels, stride, mean, pred_xstart, true, log_variance, variance, learn);
        return;
    }
    const float* c = coef + (size_t)ti * DDPM3D_NCOEF;
    const float c_recip = c[DDPM3D_C_SQRT_RECIP_ACP], c_recipm1 = c[DDPM3D_C_SQRT_RECIPM1_ACP];
    const float c1 = c[DDPM3D_C_POST_MEAN_COEF1], c2 = c[DDPM3D_C_POST_MEAN_COEF2];
    const float min_log = c[DDPM3D_C_MIN_LOG], max_log = c[DDPM3D_C_MAX_LOG];
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += stride) {
        const size_t i = (size_t)n * voxels + v;
        const float xv = x[i];
        const float x0 = step_x0(xv, mo[((size_t)n * ch) * voxels + v], c_recip, c_recipm1, flags);
        mean[i] = c1 * x0 + c2 * xv;                                    // :312-314, :216-219
        pred_xstart[i] = x0;
        if (learn) {
            const float lv = learned_logvar(mo[((size_t)n * ch + 1) * voxels + v], min_log, max_log);
            log_variance[i] = lv;
            variance[i] = expf(lv);                                     // :276
        }
    }
}

// x_t -> x_{t+1} along the deterministic DDIM ODE (:587-623).  alphas_cumprod_next[t] is alphas_cumprod[t + 1] in
// fp64 (0 at t = T - 1), so its fp32 value is the ACP column of row t + 1: no table of its own.  Reads only the eps
// half of model_out.
__global__ __launch_bounds__(256) void ddim_reverse_step_kernel(
    const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ coef,
    const int64_t* __restrict__ t_idx, int voxels, int T, int flags, float* __restrict__ sample,
    float* __restrict__ pred_xstart) {
    const int n = blockIdx.y;
    const int64_t ti = t_idx[n];
    const int ch = (flags & DDPM3D_F_LEARN_SIGMA) ? 2 : 1;
    const int stride = gridDim.x * blockDim.x;
    if (ti < 0 || ti >= T) {
        step_nan_fill(n, voxels, stride, sample, pred_xstart, pred_xstart != nullptr, nullptr, nullptr, false);
        return;
    }
    const float* c = coef + (size_t)ti * DDPM3D_NCOEF;
    const float c_recip = c[DDPM3D_C_SQRT_RECIP_ACP], c_recipm1 = c[DDPM3D_C_SQRT_RECIPM1_ACP];
    const float ab_next = ti + 1 < T ? coef[(size_t)(ti + 1) * DDPM3D_NCOEF + DDPM3D_C_ACP] : 0.0f;
    const float s_next = sqrtf(ab_next), s_next_1m = sqrtf(1.0f - ab_next);
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += stride) {
        const size_t i = (size_t)n * voxels + v;
        const float xv = x[i];
        const float x0 = step_x0(xv, mo[((size_t)n * ch) * voxels + v], c_recip, c_recipm1, flags);
        const float eps = eps_from_x0(xv, x0, c_recip, c_recipm1);      // :611-614
        sample[i] = x0 * s_next + s_next_1m * eps;                      // :615-621
        if (pred_xstart != nullptr) pred_xstart[i] = x0;
    }
}

hipError_t ddpm3d_launch_p_mean_variance(const float* mo, const float* x, const float* coef, const int64_t* t_idx,
                                         int N, int voxels, int T, int flags, float* mean, float* variance,
                                         float* log_variance, float* pred_xstart, hipStream_t st) {
    hipLaunchKernelGGL(p_mean_variance_kernel, step_grid(N, voxels), dim3(256), 0, st, mo, x, coef, t_idx, voxels, T,
                       flags, mean, variance, log_variance, pred_xstart);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_ddim_reverse_step(const float* mo, const float* x, const float* coef, const int64_t* t_idx,
                                           int N, int voxels, int T, int flags, float* sample, float* pred_xstart,
                                           hipStream_t st) {
    hipLaunchKernelGGL(ddim_reverse_step_kernel, step_grid(N, voxels), dim3(256), 0, st, mo, x, coef, t_idx, voxels,
                       T, flags, sample, pred_xstart);
    return hipGetLastError();
}

// ------------------------------------------------- DPM-Solver++ multistep step
// One step of DPM-Solver++ (Lu et al. 2022, arXiv:2211.01095): x0 from step_x0, then the update as a weighted sum
// whose weights the host expanded in fp64 into row t of scoef ([T][DDPM3D_NSCOEF]: c_x, w0, w1, w2, c_z), summed in
// that order.  m1 is read only at order >= 2, m2 only at order 3, z only when noise is non-null.  A sample whose t
// lies outside [0, T) reads neither table and gets NaN.
template <class Noise, bool X0 = false>
__global__ __launch_bounds__(256) void dpm_solver_step_kernel(
    const float* __restrict__ mo, const float* __restrict__ xs, const float* __restrict__ x,
    const float* __restrict__ m1,
    const float* __restrict__ m2, const Noise noise, const float* __restrict__ coef,
    const float* __restrict__ scoef, const int64_t* __restrict__ t_idx, int voxels, int T, int flags, int order,
    float* __restrict__ sample, float* __restrict__ pred_xstart) {
    const int n = blockIdx.y;
    const int64_t ti = t_idx[n];
    const int ch = (flags & DDPM3D_F_LEARN_SIGMA) ? 2 : 1;
    const int stride = gridDim.x * blockDim.x;
    const auto z = noise.sample(n);
    if (ti < 0 || ti >= T || !z.ok()) {
        step_nan_fill(n, voxels, stride, sample, pred_xstart, true, nullptr, nullptr, false);
        return;
    }
    const bool has_z = noise.present();
    const float* c = coef + (size_t)ti * DDPM3D_NCOEF;
    const float c_recip = c[DDPM3D_C_SQRT_RECIP_ACP], c_recipm1 = c[DDPM3D_C_SQRT_RECIPM1_ACP];
    const float* w = scoef + (size_t)ti * DDPM3D_NSCOEF;
    const float c_x = w[DDPM3D_S_CX], w0 = w[DDPM3D_S_W0], w1 = w[DDPM3D_S_W1], w2 = w[DDPM3D_S_W2];
    const float c_z = w[DDPM3D_S_CZ];
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += stride) {
        const size_t i = (size_t)n * voxels + v;
        const float xv = x[i];
        const float x0 = step_x0_from<X0>(mo, xs, i, ((size_t)n * ch) * voxels + v, xv, c_recip, c_recipm1, flags);
        float out = c_x * xv + w0 * x0;
        if (order >= 2) out = out + w1 * m1[i];
        if (order >= 3) out = out + w2 * m2[i];
        if (has_z) out = out + c_z * z.at(i, v);
        sample[i] = out;
        pred_xstart[i] = x0;
    }
}

hipError_t ddpm3d_launch_dpm_solver_step(const float* mo, const float* xs, const float* x, const float* m1,
                                         const float* m2, const float* noise, const ddpm3d_noise_key* key,
                                         const float* coef, const float* scoef, const int64_t* t_idx, int N, int voxels,
                                         int T, int flags, int order, float* sample, float* pred_xstart,
                                         hipStream_t st) {
    return launch_step(noise, key, [&](auto z, auto has_x0) {
        hipLaunchKernelGGL((dpm_solver_step_kernel<decltype(z), has_x0.value>), step_grid(N, voxels), dim3(256), 0, st,
                           mo, xs, x, m1, m2, z, coef, scoef, t_idx, voxels, T, flags, order, sample, pred_xstart);
    }, xs != nullptr);
}

// ------------------------------------------------------- variational bound
// calc_bpd_loop's per-step work after the network call (gaussian_diffusion.py:709-742, :872-880) and its helpers
// (q_sample :188-206, _prior_bpd :821-837, losses.py normal_kl / discretized_gaussian_log_likelihood).  Every element
// follows the reference's fp32 expression order (contraction is still off here).  Per-sample means: each of
// ddpm3d_vb_parts(voxels) workgroups sums a fixed slice of the volume in fp64 and writes one 32-byte record
// {term, xstart sq, eps sq, 0} to the caller's workspace; a second launch folds the records of a sample in a fixed
// order.  No atomics: the same bits on every run, whatever the launch order.
#define VB_THREADS 256
#define VB_UNROLL 4                  // elements per thread per pass, loads issued together
#define VB_MAX_PARTS 1024
#define VB_REC 4                     // doubles per record

int ddpm3d_vb_parts(int voxels) {
    const int per = VB_THREADS * VB_UNROLL;
    const int p = voxels / per + (voxels % per != 0);
    return p < VB_MAX_PARTS ? p : VB_MAX_PARTS;
}

// The voxels [v0, v1) that workgroup `part` of `parts` sums: equal chunks, the last one short.
__device__ __forceinline__ void vb_chunk(int voxels, int parts, int part, long long& v0, long long& v1) {
    const int chunk = voxels / parts + (voxels % parts != 0);
    v0 = (long long)part * chunk;
    v1 = v0 + chunk < voxels ? v0 + chunk : voxels;
}

template <class Noise>
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const Noise noise,
                                                       const float* __restrict__ qcoef,
                                                       const int64_t* __restrict__ t_idx, int voxels, int T,
                                                       float* __restrict__ xt) {
    const int n = blockIdx.y;
    const int64_t ti = t_idx[n];
    const auto z = noise.sample(n);
    if (!z.ok()) {                                // a keyed patch that leaves its canvas
        step_nan_fill(n, voxels, gridDim.x * blockDim.x, xt, nullptr, false, nullptr, nullptr, false);
        return;
    }
    float a = __builtin_nanf(""), b = a;          // t outside [0, T): no table row is read, x_t is NaN
    if (ti >= 0 && ti < T) {
        a = qcoef[(size_t)ti * DDPM3D_NQCOEF + DDPM3D_Q_SQRT_ACP];
        b = qcoef[(size_t)ti * DDPM3D_NQCOEF + DDPM3D_Q_SQRT_1M_ACP];
    }
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += gridDim.x * blockDim.x) {
        const size_t i = (size_t)n * voxels + v;
        xt[i] = a * x0[i] + b * z.at(i, v);         // :202-206
    }
}

// exp / log / tanh of an fp32 value evaluated in fp64 and rounded once: the correctly rounded fp32 result, which the
// reference's <=1-ulp fp32 libm returns almost always.  The bound's terms cancel (-1 + lv2 - lv1 + exp(lv1 - lv2) is
// ~1e-6 at the last steps), so an ulp of a fast fp32 exp would be a per-cent of a term; fp64 VALU work is free here.
__device__ __forceinline__ float exp_r(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float log_r(float x) { return (float)log((double)x); }

// losses.py approx_standard_normal_cdf.  th.pow(x, 3) is x * x * x; the double constants reach the fp32 ops rounded
// to fp32, as torch applies a Python scalar to a float tensor.
__device__ __forceinline__ float approx_std_normal_cdf(float x) {
    const float u = (float)0.7978845608028654 * (x + (float)0.044715 * (x * x * x));
    return 0.5f * (1.0f + (float)tanh((double)u));
}

// A record is {term, xstart sq, eps sq} and an explicit 0.0 in its fourth double (record_reduce.h).  The wave totals
// are folded from the first wave's, where this file once started from 0.0: the same bits, because every per-thread
// accumulator starts at +0.0 and so no partial sum can be -0.0 (the one value 0.0 + x would change).
using VbCols = RrSum<3, VB_REC>;

__global__ __launch_bounds__(VB_THREADS) void vb_terms_kernel(
    const float* __restrict__ mo, const float* __restrict__ xs_p, const float* __restrict__ xt_p,
    const float* __restrict__ noise, const float* __restrict__ coef, const float* __restrict__ qcoef,
    const int64_t* __restrict__ t_idx, int voxels, int T, int flags, int parts, double* __restrict__ slab,
    float* __restrict__ pred_xstart) {
    const int n = blockIdx.y, part = blockIdx.x;
    const int64_t ti = t_idx[n];
    double s_vb = 0.0, s_x0 = 0.0, s_eps = 0.0;
    if (ti >= 0 && ti < T) {
        const float* c = coef + (size_t)ti * DDPM3D_NCOEF;
        const float c_recip = c[DDPM3D_C_SQRT_RECIP_ACP], c_recipm1 = c[DDPM3D_C_SQRT_RECIPM1_ACP];
        const float c1 = c[DDPM3D_C_POST_MEAN_COEF1], c2 = c[DDPM3D_C_POST_MEAN_COEF2];
        const float min_log = c[DDPM3D_C_MIN_LOG], max_log = c[DDPM3D_C_MAX_LOG];
        const float true_log = qcoef[(size_t)ti * DDPM3D_NQCOEF + DDPM3D_Q_POST_LOG_VAR];
        const bool learn = flags & DDPM3D_F_LEARN_SIGMA;
        const int ch = learn ? 2 : 1;
        const float BIN = (float)(1.0 / 255.0);
        long long v0, v1;
        vb_chunk(voxels, parts, part, v0, v1);
        for (long long base = v0; base < v1; base += VB_THREADS * VB_UNROLL) {
#pragma unroll
            for (int j = 0; j < VB_UNROLL; ++j) {
                const long long v = base + j * VB_THREADS + threadIdx.x;
                if (v >= v1) continue;
                const size_t i = (size_t)n * voxels + v;
                const float xv = xt_p[i], xs = xs_p[i];
                // p_mean_variance (:262-318)
                const float x0 = step_x0(xv, mo[((size_t)n * ch) * voxels + v], c_recip, c_recipm1, flags);
                float logvar = min_log;
                if (learn) logvar = learned_logvar(mo[((size_t)n * ch + 1) * voxels + v], min_log, max_log);
                const float mean = c1 * x0 + c2 * xv;
                float term;
                if (ti == 0) {
                    // -discretized_gaussian_log_likelihood(x_start, mean, 0.5 * logvar)  (losses.py)
                    const float centered = xs - mean;
                    const float inv_stdv = exp_r(-(0.5f * logvar));
                    const float cdf_plus = approx_std_normal_cdf(inv_stdv * (centered + BIN));
                    const float cdf_min = approx_std_normal_cdf(inv_stdv * (centered - BIN));
                    float lp;
                    if (xs < -0.999f) lp = log_r(clamp_min(cdf_plus, 1e-12f));
                    else if (xs > 0.999f) lp = log_r(clamp_min(1.0f - cdf_min, 1e-12f));
                    else lp = log_r(clamp_min(cdf_plus - cdf_min, 1e-12f));
                    term = -lp;
                } else {
                    // normal_kl(true posterior mean, posterior_log_variance_clipped, mean, logvar)  (:723-728)
                    const float tmean = c1 * xs + c2 * xv;
                    const float d = tmean - mean;
                    term = 0.5f * ((((-1.0f + logvar) - true_log) + exp_r(true_log - logvar)) + (d * d) * exp_r(-logvar));
                }
                s_vb += (double)term;
                const float dx = x0 - xs;                                   // :877
                s_x0 += (double)(dx * dx);
                if (noise != nullptr) {
                    const float eps = eps_from_x0(xv, x0, c_recip, c_recipm1);   // :879
                    const float de = eps - noise[i];
                    s_eps += (double)(de * de);
                }
                if (pred_xstart != nullptr) pred_xstart[i] = x0;
            }
        }
    } else {
        s_vb = s_x0 = s_eps = __builtin_nan("");
    }
    double rec[3] = {s_vb, s_x0, s_eps};
    rr_write_record<VbCols, VB_THREADS>(rec, slab + ((size_t)n * parts + part) * VB_REC);
}

// _prior_bpd: normal_kl(sqrt_acp[T-1] * x_start, log_1m_acp[T-1], 0, 0) per element; with mean2 = logvar2 = 0 the
// reference's expression is 0.5 * (((-1 - lv) + exp(lv)) + m * m) exactly (x - 0 = x, exp(-0) = 1).
__global__ __launch_bounds__(VB_THREADS) void prior_bpd_kernel(const float* __restrict__ xs_p,
                                                               const float* __restrict__ qcoef, int voxels, int T,
                                                               int parts, double* __restrict__ slab) {
    const int n = blockIdx.y, part = blockIdx.x;
    const float sa = qcoef[(size_t)(T - 1) * DDPM3D_NQCOEF + DDPM3D_Q_SQRT_ACP];
    const float lv = qcoef[(size_t)(T - 1) * DDPM3D_NQCOEF + DDPM3D_Q_LOG_1M_ACP];
    double s = 0.0;
    long long v0, v1;
    vb_chunk(voxels, parts, part, v0, v1);
    for (long long base = v0; base < v1; base += VB_THREADS * VB_UNROLL) {
#pragma unroll
        for (int j = 0; j < VB_UNROLL; ++j) {
            const long long v = base + j * VB_THREADS + threadIdx.x;
            if (v >= v1) continue;
            const float m = sa * xs_p[(size_t)n * voxels + v];
            s += (double)(0.5f * (((-1.0f - lv) + exp_r(lv)) + m * m));
        }
    }
    double rec[3] = {s, 0.0, 0.0};
    rr_write_record<VbCols, VB_THREADS>(rec, slab + ((size_t)n * parts + part) * VB_REC);
}

// One workgroup per sample: the sample's records in a fixed order, then mean (/ ln 2 for the bound's term).
__global__ __launch_bounds__(256) void vb_fold_kernel(const double* __restrict__ slab, int parts, double count,
                                                      float* __restrict__ vb, float* __restrict__ xstart_mse,
                                                      float* __restrict__ mse, int ld) {
    const int n = blockIdx.x;
    double s[3];
    rr_fold<VbCols, 256>(slab + (size_t)n * parts * VB_REC, parts, s);
    const auto total = rr_reduce<VbCols, 256>(s);
    if (threadIdx.x == 0) {
        vb[(size_t)n * ld] = (float)(total(0) / count / 0.69314718055994530942);   // mean_flat(.) / np.log(2.0)
        if (xstart_mse != nullptr) xstart_mse[(size_t)n * ld] = (float)(total(1) / count);
        if (mse != nullptr) mse[(size_t)n * ld] = (float)(total(2) / count);
    }
}

hipError_t ddpm3d_launch_q_sample(const float* x0, const float* noise, const ddpm3d_noise_key* key, const float* qcoef,
                                  const int64_t* t_idx, int N, int voxels, int T, float* xt, hipStream_t st) {
    return launch_step(noise, key, [&](auto z) {
        hipLaunchKernelGGL(q_sample_kernel<decltype(z)>, step_grid(N, voxels), dim3(256), 0, st, x0, z, qcoef, t_idx,
                           voxels, T, xt);
    });
}

hipError_t ddpm3d_launch_vb_terms(const float* mo, const float* x_start, const float* x_t, const float* noise,
                                  const float* coef, const float* qcoef, const int64_t* t_idx, int N, int voxels,
                                  int T, int flags, double* ws, float* vb, float* xstart_mse, float* mse, int ld,
                                  float* pred_xstart, hipStream_t st) {
    const int parts = ddpm3d_vb_parts(voxels);
    hipLaunchKernelGGL(vb_terms_kernel, dim3(parts, N), dim3(VB_THREADS), 0, st, mo, x_start, x_t, noise, coef, qcoef,
                       t_idx, voxels, T, flags, parts, ws, pred_xstart);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vb_fold_kernel, dim3(N), dim3(256), 0, st, ws, parts, (double)voxels, vb, xstart_mse, mse, ld);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_prior_bpd(const float* x_start, const float* qcoef, int N, int voxels, int T, double* ws,
                                   float* out, hipStream_t st) {
    const int parts = ddpm3d_vb_parts(voxels);
    hipLaunchKernelGGL(prior_bpd_kernel, dim3(parts, N), dim3(VB_THREADS), 0, st, x_start, qcoef, voxels, T, parts, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vb_fold_kernel, dim3(N), dim3(256), 0, st, ws, parts, (double)voxels, out, nullptr, nullptr, 1);
    return hipGetLastError();
}
