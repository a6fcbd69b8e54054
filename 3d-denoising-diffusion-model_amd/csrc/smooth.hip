// Separable Gaussian post-filter (definitions in include/ddpm3d.h): the clinic's baseline denoiser.
// One launch per axis with a radius above 0, in the order W, H, D; a pass with radius 0 is the identity and is not
// launched.  The passes chain vol -> ... -> out through the caller's workspace (one volume), so that vol is only read
// and the last pass writes out: 1 pass vol -> out, 2 passes vol -> ws -> out, 3 passes vol -> out -> ws -> out; with no
// pass at all out is a device-to-device copy of vol.  A thread owns one output voxel and adds its counted taps in
// ascending order of the offset, the first as a product and the others by fma (one rounding per tap); the divisor is
// the fp64 sum of the counted taps rounded once, taken from a prefix table the host builds.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "smooth_pass.h"

namespace {

__global__ __launch_bounds__(SMOOTH_THREADS) void gauss_pass_kernel(const float* __restrict__ in,
                                                                    float* __restrict__ out, const SmoothArgs a) {
    __shared__ double s_prefix[SMOOTH_TAPS + 1];
    smooth_stage_prefix(a, s_prefix);
    const int64_t i = (int64_t)blockIdx.x * SMOOTH_THREADS + threadIdx.x;
    if (i >= a.voxels) return;
    out[i] = smooth_pass_value(a, s_prefix, i, [&](int64_t k) { return in[k]; });
}

}  // namespace

hipError_t ddpm3d_launch_gauss_smooth(const float* vol, int D, int H, int W, const int* radii, const float* const* taps,
                                      float* out, float* ws, hipStream_t st) {
    const int64_t voxels = (int64_t)D * H * W;
    // pass order W, H, D
    const int axis_r[3] = {radii[2], radii[1], radii[0]};
    const float* axis_t[3] = {taps[2], taps[1], taps[0]};
    const int64_t axis_stride[3] = {1, W, (int64_t)H * W};
    const int axis_len[3] = {W, H, D};
    int passes = 0;
    for (int k = 0; k < 3; ++k) passes += axis_r[k] > 0;
    if (passes == 0) return hipMemcpyAsync(out, vol, (size_t)voxels * sizeof(float), hipMemcpyDeviceToDevice, st);
    // the destinations of the passes, chosen so that the last is out
    float* dst[3] = {out, out, out};
    if (passes == 2) dst[0] = ws;
    if (passes == 3) dst[1] = ws;
    const float* src = vol;
    int done = 0;
    for (int k = 0; k < 3; ++k) {
        if (axis_r[k] == 0) continue;
        SmoothArgs a;
        a.voxels = voxels, a.stride = axis_stride[k], a.L = axis_len[k];
        smooth_args_taps(a, axis_r[k], axis_t[k]);
        const unsigned blocks = (unsigned)((voxels + SMOOTH_THREADS - 1) / SMOOTH_THREADS);   // at most 2^23
        hipLaunchKernelGGL(gauss_pass_kernel, dim3(blocks), dim3(SMOOTH_THREADS), 0, st, src, dst[done], a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        src = dst[done++];
    }
    return hipSuccess;
}
