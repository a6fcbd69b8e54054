// Rotating maximum-intensity and ray-sum projections (definitions in include/ddpm3d.h): an
// interpolating ray march, the library's one gather.  The rotation is about D, so a ray stays in one (H, W) slice and
// a sample is a bilinear interpolant of four voxels of that slice.  A thread owns one ray (b, angle, d, u) and walks
// its samples in ascending j, so the sum has one order and needs no atomics.  The 64 lanes of a wave are 64
// neighbouring bins of one angle: at small angles they read neighbouring addresses of one row.  The waves of a
// workgroup take the angles of a group in turn over the same slice and strip, and the workgroups of one slice are
// neighbours in the grid, so the slice comes from HBM once and is served to the other angles from cache.
// The coordinate table travels in the kernel arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int PROJECT_THREADS = 256;                    // four waves
constexpr int PROJECT_WAVES = PROJECT_THREADS / 64;
constexpr int PROJECT_GROUP = 2 * PROJECT_WAVES;        // angles a workgroup walks over its slice and strip

struct ProjectArgs {
    int B, D, H, W, strips, groups;
    ddpm3d_project_table t;
};

// Narrows [jlo, jhi] to the samples whose coordinate c0 + j m can lie in [0, len - 1].  It only ever drops samples
// that cannot count: the window is [-1, len], a voxel wider per side than the counting rule's, and two samples wider
// per end, against a coordinate that differs from the marched one by its roundings (below 2^-9 voxel for tables of
// this size) and quotients good to a few ulp of at most 2^14.  Every sample that stays is still tested by the rule.
__device__ inline void project_clip(float c0, float m, float len, int& jlo, int& jhi) {
    if (fabsf(m) * 8192.0f < 0.5f) {                    // drifts less than half a voxel over any ray
        if (!(c0 >= -1.0f && c0 <= len)) jhi = -1;
        return;
    }
    const float a = (-1.0f - c0) / m, b = (len - c0) / m;
    const float lo = fminf(fmaxf(fminf(a, b), -4.0f), 16384.0f), hi = fminf(fmaxf(fmaxf(a, b), -4.0f), 16384.0f);
    jlo = max(jlo, (int)floorf(lo) - 2);
    jhi = min(jhi, (int)ceilf(hi) + 2);
}

template <int MODE>
__global__ __launch_bounds__(PROJECT_THREADS) void project_kernel(const float* __restrict__ vol,
                                                                  float* __restrict__ out, const ProjectArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = blockIdx.x % p.strips, d = blockIdx.x / p.strips;
    const int group = blockIdx.y, b = blockIdx.z;
    const int u = strip * 64 + lane;
    if (u >= p.t.bins) return;
    const int H = p.H, W = p.W, R = p.t.samples;
    const float* __restrict__ slice = vol + ((int64_t)b * p.D + d) * ((int64_t)H * W);
    const float fu = (float)u, h_top = (float)(H - 1), w_top = (float)(W - 1), step = p.t.step;
    const int a_end = min(p.t.angles, (group + 1) * PROJECT_GROUP);
    for (int a = group * PROJECT_GROUP + wave; a < a_end; a += PROJECT_WAVES) {
        const float h0 = p.t.coef[a][0], hu = p.t.coef[a][1], hj = p.t.coef[a][2];
        const float w0 = p.t.coef[a][3], wu = p.t.coef[a][4], wj = p.t.coef[a][5];
        int jlo = 0, jhi = R - 1;
        project_clip(fmaf(fu, hu, h0), hj, (float)H, jlo, jhi);
        project_clip(fmaf(fu, wu, w0), wj, (float)W, jlo, jhi);
        float best = -__builtin_inff(), acc = 0.0f;
        bool counted = false, poisoned = false;
        for (int j = jlo; j <= jhi; ++j) {
            const float fj = (float)j;
            const float hc = fmaf(fu, hu, fmaf(fj, hj, h0));
            const float wc = fmaf(fu, wu, fmaf(fj, wj, w0));
            if (!(hc >= 0.0f && hc <= h_top && wc >= 0.0f && wc <= w_top)) continue;
            const float hf = floorf(hc), wf = floorf(wc);
            const int y0 = (int)hf, x0 = (int)wf;
            const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
            const float fy = hc - hf, fx = wc - wf;         // both exact
            const float* __restrict__ r0 = slice + (int64_t)y0 * W;
            const float* __restrict__ r1 = slice + (int64_t)y1 * W;
            const float v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
            const float top = fmaf(fx, v01 - v00, v00);
            const float bot = fmaf(fx, v11 - v10, v10);
            const float v = fmaf(fy, bot - top, top);
            if (MODE == DDPM3D_PROJECT_MAX) {
                counted = true;
                poisoned |= v != v;
                best = fmaxf(best, v);                      // drops a NaN: `poisoned` keeps it
            } else {
                acc = fmaf(step, v, acc);
            }
        }
        float r;
        if (MODE == DDPM3D_PROJECT_MAX)
            r = poisoned ? __builtin_nanf("") : (counted ? best : 0.0f);
        else
            r = acc;
        out[(((int64_t)b * p.t.angles + a) * p.D + d) * p.t.bins + u] = r;
    }
}

}  // namespace

hipError_t ddpm3d_launch_project(const float* vol, int B, int D, int H, int W, const ddpm3d_project_table& table,
                                 int mode, float* out, hipStream_t st) {
    ProjectArgs p;
    p.B = B, p.D = D, p.H = H, p.W = W;
    p.strips = (table.bins + 63) / 64;
    p.groups = (table.angles + PROJECT_GROUP - 1) / PROJECT_GROUP;
    p.t = table;
    // D * strips <= D * bins <= 2^31 - 1 (the caller has checked the output's size); groups <= 8, B <= 64
    const dim3 grid((unsigned)((int64_t)D * p.strips), (unsigned)p.groups, (unsigned)B);
    if (mode == DDPM3D_PROJECT_MAX)
        hipLaunchKernelGGL(project_kernel<DDPM3D_PROJECT_MAX>, grid, dim3(PROJECT_THREADS), 0, st, vol, out, p);
    else
        hipLaunchKernelGGL(project_kernel<DDPM3D_PROJECT_SUM>, grid, dim3(PROJECT_THREADS), 0, st, vol, out, p);
    return hipGetLastError();
}
