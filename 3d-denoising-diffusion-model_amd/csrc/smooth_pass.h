// One pass of the separable Gaussian with renormalised faces (include/ddpm3d.h, ddpm3d_gauss_smooth): the per-voxel
// rule that smooth.hip's post-filter and guide.hip's x_start pull share, so that both give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"

constexpr int SMOOTH_THREADS = 256;
constexpr int SMOOTH_TAPS = 2 * DDPM3D_SMOOTH_MAX_RADIUS + 1;

struct SmoothArgs {
    int64_t voxels;
    int64_t stride;                                           // words between neighbours along the pass's axis
    int L;                                                    // the extent along it
    int r;
    float taps[SMOOTH_TAPS];                                  // taps[j + r], j = -r..r
    double prefix[SMOOTH_TAPS + 1];                           // prefix[k] = taps[0] + ... + taps[k - 1] in fp64
};

// the taps of one axis (2 r + 1 of them) and their fp64 prefix sums
static inline void smooth_args_taps(SmoothArgs& a, int r, const float* taps) {
    a.r = r;
    const int n = 2 * r + 1;
    a.prefix[0] = 0.0;
    for (int j = 0; j < SMOOTH_TAPS; ++j) {
        a.taps[j] = j < n ? taps[j] : 0.0f;
        a.prefix[j + 1] = a.prefix[j] + (double)a.taps[j];
    }
}

// the workgroup's copy of the prefix table: read with a per-lane index at the faces
__device__ __forceinline__ void smooth_stage_prefix(const SmoothArgs& a, double* s_prefix) {
    for (int i = threadIdx.x; i <= 2 * a.r + 1; i += SMOOTH_THREADS) s_prefix[i] = a.prefix[i];
    __syncthreads();
}

// Voxel i of one volume: the counted taps in ascending order of the offset, the first as a product and the others by
// fma (one rounding per tap), over the fp64 sum of the counted taps rounded once.  load(k) is the pass's input at voxel k.
template <class Load>
__device__ __forceinline__ float smooth_pass_value(const SmoothArgs& a, const double* s_prefix, int64_t i, Load load) {
    const int c = (int)((i / a.stride) % a.L);
    const int lo = c < a.r ? -c : -a.r, hi = a.L - 1 - c < a.r ? a.L - 1 - c : a.r;   // the counted offsets
    float acc = 0.0f;
    for (int j = -a.r; j <= a.r; ++j) {                       // the same trip count for all lanes; taps[] is scalar
        const bool counted = j >= lo && j <= hi;
        const float x = counted ? load(i + (int64_t)j * a.stride) : 0.0f;
        const float t = a.taps[j + a.r];
        const float next = j == lo ? t * x : __builtin_fmaf(t, x, acc);
        acc = counted ? next : acc;
    }
    const float den = (float)(s_prefix[hi + a.r + 1] - s_prefix[lo + a.r]);
    return acc / den;
}
