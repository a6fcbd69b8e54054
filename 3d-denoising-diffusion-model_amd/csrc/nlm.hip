// Non-local means (definitions in include/ddpm3d.h): out[v] = sum_s w(v, s) x[v + s] / sum_s w(v, s)
// over the search box, w from the mean squared difference of the patches around v and v + s.  One launch on the
// halo-tile frame of halo_tile.h (tiles, staging, grid and launch are there): the halo of s_a + p_a per side is staged
// with replicate padding (the coordinate clamped into the volume: what a patch tap reads; a candidate outside the
// volume is dropped by its coordinate, not by what is staged).  A thread owns the TD outputs above one another at
// (y, lane): for one candidate offset and one (py, px) it reads the two columns of TD + 2 p0 words once, forms the
// TD + 2 p0 differences and adds their squares to the TD sums in the order pz = -p0..p0, so a column's words serve
// 2 p0 + 1 patch taps each.  The order of every sum is fixed: patch taps (py, px, pz) ascending, candidates in raster
// order of s; it depends on neither the tile nor the place of the voxel in it.  No atomics; plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "halo_tile.h"

namespace {

constexpr int NLM_MAX_HALO = DDPM3D_NLM_MAX_SEARCH + DDPM3D_NLM_MAX_PATCH;
constexpr size_t NLM_LDS_TWO = 80 * 1024;                     // a tile this small leaves room for two workgroups per CU
constexpr int NLM_TILES[5][2] = {{8, 8}, {8, 4}, {4, 4}, {2, 4}, {1, 4}};    // in order of preference (halo_pick)

struct NlmArgs {
    int D, H, W;
    int s0, s1, s2, p0, p1, p2;
    int TH;
    float k1, k2;                                             // a = max(fma(sum of squares, k1, -k2), 0)
};

constexpr size_t nlm_lds_bytes(int TD, int TH, int R0, int R1, int R2) {
    return halo_words(TD, TH, R0, R1, R2) * sizeof(float);
}
static_assert(nlm_lds_bytes(NLM_TILES[4][0], NLM_TILES[4][1], NLM_MAX_HALO, NLM_MAX_HALO, NLM_MAX_HALO) <= HALO_LDS_ALL,
              "the smallest tile of the largest windows fits a CU's LDS");
static_assert(2 * NLM_MAX_HALO <= HALO_TW, "a staged row is at most two words per lane");

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t hi) { return v < 0 ? 0 : v > hi ? hi : v; }

template <int TD>
__global__ __launch_bounds__(HALO_THREADS) void nlm_kernel(const float* __restrict__ vol, float* __restrict__ out,
                                                          const NlmArgs a) {
    extern __shared__ float sx[];
    constexpr int COL = TD + 2 * DDPM3D_NLM_MAX_PATCH;        // the longest column of differences
    const int R0 = a.s0 + a.p0, R1 = a.s1 + a.p1, R2 = a.s2 + a.p2;
    const HaloFrame f = halo_frame(TD, a.TH, R0, R1, R2, a.D, a.H, a.W);
    const auto [LW, LH, LD, slab, lane, wave, tiles_w, tiles_d, tx0, ty0, plane] = f;   // the compute loop's names
    const int64_t x = tx0 + lane;
    const int col = TD + 2 * a.p0;

    for (int tz = blockIdx.y; tz < tiles_d; tz += gridDim.y) {
        const int64_t tz0 = (int64_t)tz * TD;
        // stage with every coordinate clamped into the volume, so every load is in bounds
        const int64_t gx0 = clampi(tx0 - R2 + lane, a.W - 1), gx1 = clampi(tx0 - R2 + lane + 64, a.W - 1);
        halo_stage<float>(
            f, 2 * R2,
            [&](int row, float& v0, float& v1) {
                row = row < f.LD * f.LH ? row : f.LD * f.LH - 1;
                const int64_t gz = clampi(tz0 - R0 + row / f.LH, a.D - 1), gy = clampi(f.ty0 - R1 + row % f.LH, a.H - 1);
                const int64_t at = gz * f.plane + gy * a.W;
                v0 = vol[at + gx0];
                v1 = vol[at + gx1];
            },
            [&](int at, float v) { sx[at] = v; });
        __syncthreads();

        for (int oy = wave; oy < a.TH; oy += HALO_THREADS / 64) {
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

template <int TD>
constexpr auto nlm_launch = halo_launch<nlm_kernel<TD>, const float*, float*, NlmArgs>;

HaloPick nlm_tile(int R0, int R1, int R2) {
    return halo_pick(NLM_TILES, NLM_LDS_TWO, 0, [=](int TD, int TH) { return nlm_lds_bytes(TD, TH, R0, R1, R2); });
}

}  // namespace

hipError_t ddpm3d_launch_nlm(const float* vol, int D, int H, int W, const int* search, const int* patch, float k1,
                             float k2, float* out, hipStream_t st) {
    NlmArgs a;
    a.D = D, a.H = H, a.W = W;
    a.s0 = search[0], a.s1 = search[1], a.s2 = search[2];
    a.p0 = patch[0], a.p1 = patch[1], a.p2 = patch[2];
    a.k1 = k1, a.k2 = k2;
    const HaloPick tile = nlm_tile(a.s0 + a.p0, a.s1 + a.p1, a.s2 + a.p2);
    if (tile.lds_bytes == 0) return hipErrorInvalidValue;    // not reached for radii within the limits
    a.TH = tile.TH;
    const auto launch = tile.TD == 8 ? nlm_launch<8> : tile.TD == 4 ? nlm_launch<4> : tile.TD == 2 ? nlm_launch<2>
                                                                                                    : nlm_launch<1>;
    return launch(halo_grid(1, D, H, W, tile.TD, tile.TH), tile.lds_bytes, 0, st, vol, out, a);
}
