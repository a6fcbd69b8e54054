// Per-voxel order statistics of K posterior draws of one volume.
//
// draw_quantiles_kernel reads each voxel's K draws once (the same x_d = acc[d] / wsum, a correctly rounded fp32
// division, that draw_moments_kernel reduces), sorts them in registers with Batcher's odd-even merge sort of the padded
// count KP (padding +inf) and writes up to DDPM3D_MAX_QUANTILES quantiles with numpy's "linear" interpolation
// (Hyndman-Fan type 7) and, with a target, how many draws lie below and how many equal the target's value: the
// target's rank among the draws.  One thread per voxel, so every draw's load is one contiguous row per wave; the
// network is fully unrolled with compile-time indices and the run-time order index of a quantile picks its two
// neighbours by compare-and-select, so the KP values never leave the registers.  Offsets are 64-bit and every output
// element has one writer: no atomics, results are bit-repeatable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

static_assert(sizeof(ddpm3d_quantile_pos) == DDPM3D_MAX_QUANTILES * 8, "one lower and one frac per quantile");
constexpr int QN_THREADS = 256;
constexpr uint8_t QN_NOT_COUNTED = 255;    // K <= 64: no rank reaches it

// One comparator.  No NaN reaches it (the kernel sorts zeros in a voxel that has one), so min / max keep the multiset.
__device__ __forceinline__ void compare_swap(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}

// Batcher's odd-even merge sort of N = 2^m values, ascending (Knuth 5.2.2 M): 1, 3, 9, 25, 63, 191, 543 comparators for
// N = 2 .. 64.  Every loop bound is a compile-time constant, so after unrolling every index is one too.
template <int N>
__device__ __forceinline__ void sort_network(float (&s)[N]) {
#pragma unroll
    for (int p = 1; p < N; p *= 2) {
#pragma unroll
        for (int k = p; k >= 1; k /= 2) {
#pragma unroll
            for (int j = k % p; j + k < N; j += 2 * k) {
#pragma unroll
                for (int i = 0; i < k; ++i) {
                    if (i + j + k < N && (i + j) / (2 * p) == (i + j + k) / (2 * p))
                        compare_swap(s[i + j], s[i + j + k]);
                }
            }
        }
    }
}

// WEIGHTED: wsum is there and every draw is divided by it (the division is a dozen VALU instructions per draw, as many
// as the network spends on it at KP = 64: the plain stack does not pay for them).
template <int KP, bool WEIGHTED>
__global__ __launch_bounds__(QN_THREADS) void draw_quantiles_kernel(
    const float* __restrict__ acc, const float* __restrict__ wsum, int K, int64_t voxels, int nq,
    ddpm3d_quantile_pos pos, const float* __restrict__ target, float* __restrict__ quant, uint8_t* __restrict__ below,
    uint8_t* __restrict__ equal) {
    const int64_t i = (int64_t)blockIdx.x * QN_THREADS + threadIdx.x;
    if (i >= voxels) return;
    float ws = 1.0f;
    bool live = true;
    if constexpr (WEIGHTED) {
        const float w = wsum[i];
        live = w > 0.0f;
        ws = live ? w : 1.0f;
    }
    float t = 0.0f;
    bool nan_target = false, nan_draw = false;  // taken while loading: no NaN enters a comparison below
    if (target) {
        t = target[i];
        nan_target = t != t;
        t = nan_target ? 0.0f : t;
    }
    float s[KP];
    int n_below = 0, n_equal = 0;
    // Loads go out in groups of G before anything waits on them.  K > KP / 2 (K = KP = 2 aside), so the first half is
    // there for every K; a later group is skipped when it starts past K (K is uniform: a scalar branch) and reads
    // the last draw again, in bounds, where it straddles K.
    constexpr int G = KP < 8 ? KP : 8;
#pragma unroll
    for (int g = 0; g < KP; g += G) {
        if (g < KP / 2 || g < K) {
            float a[G];
#pragma unroll
            for (int e = 0; e < G; ++e) a[e] = acc[(int64_t)(g + e < K ? g + e : K - 1) * voxels + i];
#pragma unroll
            for (int e = 0; e < G; ++e) {
                const bool real = g + e < K;
                float x = WEIGHTED ? __fdiv_rn(a[e], ws) : a[e];
                const bool bad = x != x;
                nan_draw = nan_draw || bad;
                x = bad ? 0.0f : x;
                n_below += real && x < t;
                n_equal += real && x == t;
                s[g + e] = real ? x : __builtin_inff();
            }
        } else {
#pragma unroll
            for (int e = 0; e < G; ++e) s[g + e] = __builtin_inff();
        }
    }
    if (target) {
        const bool counted = live && !nan_draw && !nan_target;
        below[i] = counted ? (uint8_t)n_below : QN_NOT_COUNTED;
        equal[i] = counted ? (uint8_t)n_equal : QN_NOT_COUNTED;
    }
    if (nq == 0) return;
    sort_network<KP>(s);
#pragma unroll
    for (int q = 0; q < DDPM3D_MAX_QUANTILES; ++q) {
        if (q >= nq) break;
        const int lower = pos.lower[q];
        const float frac = pos.frac[q];
        float lo = s[0], hi = s[0];
#pragma unroll
        for (int j = 1; j < KP; ++j) {          // lower is a run-time value: select, never index
            lo = j == lower ? s[j] : lo;
            hi = j == lower + 1 ? s[j] : hi;
        }
        const float v = frac == 0.0f ? lo : fmaf(frac, hi - lo, lo);
        quant[q * voxels + i] = !live ? 0.0f : nan_draw ? __builtin_nanf("") : v;
    }
}

template <int KP>
hipError_t launch(const float* acc, const float* wsum, int K, int64_t voxels, int nq, const ddpm3d_quantile_pos& pos,
                  const float* target, float* quant, uint8_t* below, uint8_t* equal, hipStream_t st) {
    const int64_t blocks = (voxels + QN_THREADS - 1) / QN_THREADS;
    if (wsum)
        hipLaunchKernelGGL((draw_quantiles_kernel<KP, true>), dim3((unsigned)blocks), dim3(QN_THREADS), 0, st, acc,
                           wsum, K, voxels, nq, pos, target, quant, below, equal);
    else
        hipLaunchKernelGGL((draw_quantiles_kernel<KP, false>), dim3((unsigned)blocks), dim3(QN_THREADS), 0, st, acc,
                           wsum, K, voxels, nq, pos, target, quant, below, equal);
    return hipGetLastError();
}

}  // namespace

hipError_t ddpm3d_launch_draw_quantiles(const float* acc, const float* wsum, int K, int64_t voxels, int nq,
                                        const ddpm3d_quantile_pos& pos, const float* target, float* quant,
                                        uint8_t* below, uint8_t* equal, hipStream_t st) {
#define QN_CASE(KP) \
    if (K <= KP) return launch<KP>(acc, wsum, K, voxels, nq, pos, target, quant, below, equal, st)
    QN_CASE(2);
    QN_CASE(4);
    QN_CASE(8);
    QN_CASE(16);
    QN_CASE(32);
#undef QN_CASE
    return launch<64>(acc, wsum, K, voxels, nq, pos, target, quant, below, equal, st);
}
