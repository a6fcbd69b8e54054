// Non-local means (definitions in include/ddpm3d.h): out[v] = sum_s w(v, s) x[v + s] / sum_s w(v, s)
// over the search box, w from the mean squared difference of the patches around v and v + s.  One launch.  A
// workgroup of four waves owns an output tile of TD x TH x 64 voxels and stages the tile plus a halo of s_a + p_a per
// side in LDS with replicate padding (the coordinate clamped into the volume: what a patch tap reads; a candidate
// outside the volume is dropped by its coordinate, not by what is staged).  lane = x, so every LDS read of a wave is
// 64 consecutive words.  A thread owns the TD outputs above one another at (y, lane): for one candidate offset and
// one (py, px) it reads the two columns of TD + 2 p0 words once, forms the TD + 2 p0 differences and adds their
// squares to the TD sums in the order pz = -p0..p0, so a column's words serve 2 p0 + 1 patch taps each.  The order of
// every sum is fixed: patch taps (py, px, pz) ascending, candidates in raster order of s; it depends on neither the
// tile nor the place of the voxel in it.  No atomics; plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int NLM_THREADS = 256;
constexpr int NLM_TW = 64;                                    // one wave spans the tile along W
constexpr int NLM_STAGE_ROWS = 8;                             // rows a wave has in flight while staging
constexpr int NLM_MAX_HALO = DDPM3D_NLM_MAX_SEARCH + DDPM3D_NLM_MAX_PATCH;
constexpr size_t NLM_LDS_TWO = 80 * 1024;                     // a tile this small leaves room for two workgroups per CU
constexpr size_t NLM_LDS_ALL = 160 * 1024;                    // the LDS of a CU
constexpr size_t NLM_LDS_PLAIN = 64 * 1024;                   // what a launch may use without raising the kernel's limit
// tiles in order of preference: the first that fits NLM_LDS_TWO, else the first that fits NLM_LDS_ALL
constexpr int NLM_TILES[5][2] = {{8, 8}, {8, 4}, {4, 4}, {2, 4}, {1, 4}};

struct NlmArgs {
    int D, H, W;
    int s0, s1, s2, p0, p1, p2;
    int TH;
    float k1, k2;                                             // a = max(fma(sum of squares, k1, -k2), 0)
};

constexpr size_t nlm_lds_bytes(int TD, int TH, int R0, int R1, int R2) {
    return (size_t)(TD + 2 * R0) * (TH + 2 * R1) * (NLM_TW + 2 * R2) * sizeof(float);
}
static_assert(nlm_lds_bytes(NLM_TILES[4][0], NLM_TILES[4][1], NLM_MAX_HALO, NLM_MAX_HALO, NLM_MAX_HALO) <= NLM_LDS_ALL,
              "the smallest tile of the largest windows fits a CU's LDS");
static_assert(2 * NLM_MAX_HALO <= NLM_TW, "a staged row is at most two words per lane");

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// grid: x = tiles along W x tiles along H, y = tiles along D (strided: an extent may exceed a grid's y range)
template <int TD>
__global__ __launch_bounds__(NLM_THREADS) void nlm_kernel(const float* __restrict__ vol, float* __restrict__ out,
                                                          const NlmArgs a) {
    extern __shared__ float sx[];
    constexpr int COL = TD + 2 * DDPM3D_NLM_MAX_PATCH;        // the longest column of differences
    const int R0 = a.s0 + a.p0, R1 = a.s1 + a.p1, R2 = a.s2 + a.p2;
    const int LW = NLM_TW + 2 * R2, LH = a.TH + 2 * R1, LD = TD + 2 * R0;
    const int slab = LH * LW;                                 // words per staged plane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles_w = (int)(((int64_t)a.W + NLM_TW - 1) / NLM_TW);
    const int tiles_d = (int)(((int64_t)a.D + TD - 1) / TD);
    const int64_t tx0 = (int64_t)(blockIdx.x % tiles_w) * NLM_TW;
    const int64_t ty0 = (int64_t)(blockIdx.x / tiles_w) * a.TH;
    const int64_t x = tx0 + lane;
    const int64_t plane = (int64_t)a.H * a.W;
    const int col = TD + 2 * a.p0;

    for (int tz = blockIdx.y; tz < tiles_d; tz += gridDim.y) {
        const int64_t tz0 = (int64_t)tz * TD;
        // stage with every coordinate clamped into the volume, so every load is in bounds: a wave takes
        // NLM_STAGE_ROWS consecutive rows at a time, a lane the words lane and (the tail of 2 R2 words) lane + 64
        const int64_t gx0 = clampi(tx0 - R2 + lane, a.W - 1), gx1 = clampi(tx0 - R2 + lane + 64, a.W - 1);
        for (int row0 = wave * NLM_STAGE_ROWS; row0 < LD * LH; row0 += NLM_THREADS / 64 * NLM_STAGE_ROWS) {
            float v0[NLM_STAGE_ROWS], v1[NLM_STAGE_ROWS];
#pragma unroll
            for (int r = 0; r < NLM_STAGE_ROWS; ++r) {
                const int row = row0 + r < LD * LH ? row0 + r : LD * LH - 1;
                const int64_t gz = clampi(tz0 - R0 + row / LH, a.D - 1), gy = clampi(ty0 - R1 + row % LH, a.H - 1);
                const int64_t at = gz * plane + gy * a.W;
                v0[r] = vol[at + gx0];
                v1[r] = vol[at + gx1];
            }
#pragma unroll
            for (int r = 0; r < NLM_STAGE_ROWS; ++r) {
                const int row = row0 + r;
                if (row >= LD * LH) break;
                sx[row * LW + lane] = v0[r];
                if (lane < 2 * R2) sx[row * LW + 64 + lane] = v1[r];
            }
        }
        __syncthreads();

        for (int oy = wave; oy < a.TH; oy += NLM_THREADS / 64) {
            const int64_t y = ty0 + oy;
            if (y >= a.H) break;                              // the same for all lanes of the wave
            // the voxel of output j = 0 in the staged tile; output j lies j planes further on
            const int centre = (R0 * LH + oy + R1) * LW + R2 + lane;
            float num[TD], den[TD], lost[TD];                 // den + lost: a compensated (Kahan) sum of the weights
#pragma unroll
            for (int j = 0; j < TD; ++j) {
                num[j] = -0.0f;                               // -0 + x = x for every x: one candidate gives the voxel's own bits
                den[j] = 0.0f;
                lost[j] = 0.0f;
            }
            for (int sz = -a.s0; sz <= a.s0; ++sz) {
                if (tz0 + sz + TD - 1 < 0 || tz0 + sz >= a.D) continue;       // no output of the column has this candidate
                for (int sy = -a.s1; sy <= a.s1; ++sy) {
                    if (y + sy < 0 || y + sy >= a.H) continue;                // the same for all lanes
                    for (int sx_ = -a.s2; sx_ <= a.s2; ++sx_) {
                        const int cand = centre + (sz * LH + sy) * LW + sx_;
                        const bool x_in = x + sx_ >= 0 && x + sx_ < a.W;
                        const bool self = sz == 0 && sy == 0 && sx_ == 0;
                        float d2[TD];
#pragma unroll
                        for (int j = 0; j < TD; ++j) d2[j] = 0.0f;
                        for (int py = -a.p1; py <= a.p1; ++py) {
                            for (int px = -a.p2; px <= a.p2; ++px) {
                                const int off = py * LW + px - a.p0 * slab;
                                float diff[COL];
#pragma unroll
                                for (int k = 0; k < COL; ++k) {
                                    if (k >= col) break;      // the same for all lanes
                                    diff[k] = sx[centre + off + k * slab] - sx[cand + off + k * slab];
                                }
#pragma unroll
                                for (int pz = 0; pz <= 2 * DDPM3D_NLM_MAX_PATCH; ++pz) {
                                    if (pz > 2 * a.p0) break;
#pragma unroll
                                    for (int j = 0; j < TD; ++j) d2[j] = __builtin_fmaf(diff[j + pz], diff[j + pz], d2[j]);
                                }
                            }
                        }
#pragma unroll
                        for (int j = 0; j < TD; ++j) {
                            const float arg = fmaxf(__builtin_fmaf(d2[j], a.k1, -a.k2), 0.0f);
                            // beyond the cutoff the weight is exactly 0 (a NaN compares false and is dropped too)
                            float w = arg <= DDPM3D_NLM_CUTOFF ? expf(-arg) : 0.0f;
                            if (self) w = 1.0f;
                            const bool counted = x_in && tz0 + j + sz >= 0 && tz0 + j + sz < a.D && w > 0.0f;
                            const float xv = sx[cand + j * slab];
                            num[j] = counted ? __builtin_fmaf(w, xv, num[j]) : num[j];
                            // Kahan: lost carries what the last addition dropped
                            const float term = w - lost[j];
                            const float total = den[j] + term;
                            const float dropped = (total - den[j]) - term;
                            lost[j] = counted ? dropped : lost[j];
                            den[j] = counted ? total : den[j];
                        }
                    }
                }
            }
            if (x < a.W) {
#pragma unroll
                for (int j = 0; j < TD; ++j) {
                    if (tz0 + j >= a.D) break;
                    // both words of the compensated divisor enter one fp64 division: the divisor and the division
                    // cost one final rounding.  den >= 1: the voxel itself
                    out[(tz0 + j) * plane + y * a.W + x] = (float)((double)num[j] / ((double)den[j] - (double)lost[j]));
                }
            }
        }
        __syncthreads();                                      // the next tile overwrites the LDS
    }
}

hipError_t nlm_launch(int TD, const float* vol, float* out, const NlmArgs& a, dim3 grid, size_t lds_bytes,
                      hipStream_t st) {
    void (*fn)(const float*, float*, const NlmArgs) =
        TD == 8 ? nlm_kernel<8> : TD == 4 ? nlm_kernel<4> : TD == 2 ? nlm_kernel<2> : nlm_kernel<1>;
    if (lds_bytes > NLM_LDS_PLAIN) {
        // raise this instantiation's limit to all a CU has, once per device (bit d of the mask), not per launch
        static std::atomic<unsigned long long> raised[4];
        std::atomic<unsigned long long>& mask = raised[TD == 8 ? 0 : TD == 4 ? 1 : TD == 2 ? 2 : 3];
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return e;
        const unsigned long long bit = device < 64 ? 1ull << device : 0;   // beyond 64 devices: set it every time
        if (!(mask.load(std::memory_order_acquire) & bit)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)NLM_LDS_ALL);
            if (e != hipSuccess) return e;
            mask.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(fn, grid, dim3(NLM_THREADS), lds_bytes, st, vol, out, a);
    return hipGetLastError();
}

}  // namespace

void ddpm3d_nlm_tile(int R0, int R1, int R2, int* TD, int* TH, size_t* lds_bytes) {
    const size_t budgets[2] = {NLM_LDS_TWO, NLM_LDS_ALL};
    for (size_t budget : budgets) {
        for (const auto& t : NLM_TILES) {
            const size_t need = nlm_lds_bytes(t[0], t[1], R0, R1, R2);
            if (need <= budget) {
                *TD = t[0];
                *TH = t[1];
                *lds_bytes = need;
                return;
            }
        }
    }
    *TD = *TH = 0;                                            // not reached for radii within the limits
    *lds_bytes = 0;
}

hipError_t ddpm3d_launch_nlm(const float* vol, int D, int H, int W, const int* search, const int* patch, float k1,
                             float k2, float* out, hipStream_t st) {
    NlmArgs a;
    a.D = D, a.H = H, a.W = W;
    a.s0 = search[0], a.s1 = search[1], a.s2 = search[2];
    a.p0 = patch[0], a.p1 = patch[1], a.p2 = patch[2];
    a.k1 = k1, a.k2 = k2;
    int TD = 0;
    size_t lds_bytes = 0;
    ddpm3d_nlm_tile(a.s0 + a.p0, a.s1 + a.p1, a.s2 + a.p2, &TD, &a.TH, &lds_bytes);
    if (lds_bytes == 0) return hipErrorInvalidValue;
    // H * W <= 2^31 - 1, so the x extent fits; the y extent is capped and the kernel strides over the tiles along D
    const int64_t tiles_hw = (((int64_t)W + NLM_TW - 1) / NLM_TW) * (((int64_t)H + a.TH - 1) / a.TH);
    const int tiles_d = (int)(((int64_t)D + TD - 1) / TD);
    const dim3 grid((unsigned)tiles_hw, (unsigned)(tiles_d < 65535 ? tiles_d : 65535), 1);
    return nlm_launch(TD, vol, out, a, grid, lds_bytes, st);
}
