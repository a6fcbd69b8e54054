// Low-pass data-consistency pull of a step's x_start prediction (definitions in include/ddpm3d.h):
//   x0 = clip(x0_raw + w * G(y - x0_raw))
// at the position of the reference's denoised_fn (gaussian_diffusion.py:293-314).  G is ddpm3d_gauss_smooth's
// separable Gaussian (smooth_pass.h: the same per-pass rule, the same order W, H, D), batched over the samples.
// One launch per axis with a radius above 0, or one launch in all when every radius is 0.  The first pass derives
// x0_raw and the residual y - x0_raw at every tap it reads (x0_raw never reaches memory), the last pass derives
// x0_raw once more at its own voxel and finishes the pull and the clip: 1 pass -> out, 2 passes -> ws -> out,
// 3 passes -> out -> ws -> out.  A thread owns one voxel of one sample (grid row = sample) and reads that sample
// only.  No atomics, every sum in a fixed order: the same bits on every run and for every launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "smooth_pass.h"

// the expressions mirror torch's one rounding at a time, as in the step section of ops.hip
#pragma clang fp contract(off)

namespace {

struct PullArgs {
    const float* mo;
    const float* x;
    const float* y;
    const float* coef;
    const int64_t* t_idx;
    int T, flags;
    float weight;
};

// FIRST: the pass reads the residual y - x0_raw, formed where it is read; LAST: it finishes x0 from its result.
// a.r == 0 (only when no axis has a radius: FIRST and LAST) takes the residual itself.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(SMOOTH_THREADS) void pull_pass_kernel(const PullArgs p, const float* __restrict__ in,
                                                                   float* __restrict__ out, const SmoothArgs a) {
    __shared__ double s_prefix[SMOOTH_TAPS + 1];
    smooth_stage_prefix(a, s_prefix);
    const int n = blockIdx.y;
    const int64_t v = (int64_t)blockIdx.x * SMOOTH_THREADS + threadIdx.x;
    if (v >= a.voxels) return;
    const size_t base = (size_t)n * (size_t)a.voxels;
    const int64_t ti = p.t_idx[n];
    if (ti < 0 || ti >= p.T) {                                // step_nan_fill's rule: no table row is read
        out[base + v] = __builtin_nanf("");
        return;
    }
    float c_recip = 0.0f, c_recipm1 = 0.0f;
    if (FIRST || LAST) {
        const float* c = p.coef + (size_t)ti * DDPM3D_NCOEF;
        c_recip = c[DDPM3D_C_SQRT_RECIP_ACP], c_recipm1 = c[DDPM3D_C_SQRT_RECIPM1_ACP];
    }
    const int ch = (p.flags & DDPM3D_F_LEARN_SIGMA) ? 2 : 1;
    const float* mo = p.mo + base * ch;                       // the sample's first half: x_start itself, or eps
    const float* x = p.x + base;
    // step_x0 without the clip (:305-311, :328-333)
    auto raw = [&](int64_t k) {
        return (p.flags & DDPM3D_F_PREDICT_XSTART) ? mo[k] : c_recip * x[k] - c_recipm1 * mo[k];
    };
    auto src = [&](int64_t k) { return FIRST ? p.y[base + k] - raw(k) : in[base + k]; };
    const float g = a.r == 0 ? src(v) : smooth_pass_value(a, s_prefix, v, src);
    if (LAST) {
        const float wg = p.weight * g;
        float x0 = raw(v) + wg;
        // :296-297, after denoised_fn; a NaN stays NaN as in x.clamp(-1, 1) (step_x0's rule)
        if (p.flags & DDPM3D_F_CLIP) x0 = x0 < -1.0f ? -1.0f : (x0 > 1.0f ? 1.0f : x0);
        out[base + v] = x0;
    } else {
        out[base + v] = g;
    }
}

template <bool FIRST, bool LAST>
hipError_t launch_pass(const PullArgs& p, int N, const float* in, float* out, const SmoothArgs& a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.voxels + SMOOTH_THREADS - 1) / SMOOTH_THREADS);   // at most 2^23
    hipLaunchKernelGGL((pull_pass_kernel<FIRST, LAST>), dim3(blocks, N), dim3(SMOOTH_THREADS), 0, st, p, in, out, a);
    return hipGetLastError();
}

}  // namespace

hipError_t ddpm3d_launch_xstart_pull(const float* mo, const float* x, const float* y, const float* coef,
                                     const int64_t* t_idx, int N, int D, int H, int W, int T, int flags, float weight,
                                     const int* radii, const float* const* taps, float* out, float* ws,
                                     hipStream_t st) {
    const PullArgs p = {mo, x, y, coef, t_idx, T, flags, weight};
    // pass order W, H, D
    const int axis_r[3] = {radii[2], radii[1], radii[0]};
    const float* axis_t[3] = {taps[2], taps[1], taps[0]};
    const int64_t axis_stride[3] = {1, W, (int64_t)H * W};
    const int axis_len[3] = {W, H, D};
    SmoothArgs a;
    a.voxels = (int64_t)D * H * W;
    int passes = 0;
    for (int k = 0; k < 3; ++k) passes += axis_r[k] > 0;
    if (passes == 0) {                                        // the pointwise pull
        a.stride = 1, a.L = W;
        const float one = 1.0f;
        smooth_args_taps(a, 0, &one);
        return launch_pass<true, true>(p, N, nullptr, out, a, st);
    }
    // the destinations of the passes, chosen so that the last is out
    float* dst[3] = {out, out, out};
    if (passes == 2) dst[0] = ws;
    if (passes == 3) dst[1] = ws;
    const float* src = nullptr;
    int done = 0;
    for (int k = 0; k < 3; ++k) {
        if (axis_r[k] == 0) continue;
        a.stride = axis_stride[k], a.L = axis_len[k];
        smooth_args_taps(a, axis_r[k], axis_t[k]);
        const bool first = done == 0, last = done == passes - 1;
        const hipError_t e = first ? (last ? launch_pass<true, true>(p, N, src, dst[done], a, st)
                                           : launch_pass<true, false>(p, N, src, dst[done], a, st))
                                   : (last ? launch_pass<false, true>(p, N, src, dst[done], a, st)
                                           : launch_pass<false, false>(p, N, src, dst[done], a, st));
        if (e != hipSuccess) return e;
        src = dst[done++];
    }
    return hipSuccess;
}
