// Sphere-mean map for SUVpeak (definitions in include/ddpm3d.h): out[b][v] = mean of vol[b] over the
// footprint voxels around v that lie inside the volume and are kept.  One dense pass on the halo-tile frame of
// halo_tile.h (tiles, staging, grid and launch are there): the halo is staged with zeros outside the volume and where
// keep == 0, with keep also one flag byte per voxel, and the footprint's row runs are summed from LDS.  The footprint
// travels in the kernel arguments as the list of its present rows (dz, dy, half-width), which a workgroup copies to LDS
// once, so each row's half-width is a scalar.  Taps are added in one order whatever the tile: the same bits on every
// run, and row b does not depend on B.  No atomics; plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "halo_tile.h"

namespace {

constexpr int PEAK_SIDE = 2 * DDPM3D_PEAK_MAX_RADIUS + 1;
constexpr size_t PEAK_LDS_FOUR = 40 * 1024;                   // a tile this small leaves room for four workgroups per CU
constexpr size_t PEAK_LDS_STATIC = sizeof(int) * PEAK_SIDE * PEAK_SIDE;   // the row list
constexpr int PEAK_TILES[5][2] = {{8, 8}, {4, 8}, {4, 4}, {2, 4}, {1, 4}};   // in order of preference (halo_pick)

struct PeakArgs {
    int D, H, W;
    int r0, r1, rw;                                           // rw = the largest half-width of the table
    int TD, TH;
    int taps;                                                 // the whole footprint's voxel count
    int n_rows;                                               // present rows, in the order dz, dy ascending
    int rows[PEAK_SIDE * PEAK_SIDE];                          // (dz + r0) | (dy + r1) << 8 | half-width << 16
};

constexpr size_t peak_lds_bytes(int TD, int TH, int r0, int r1, int rw, bool keep) {
    const size_t n = halo_words(TD, TH, r0, r1, rw);
    return n * sizeof(float) + (keep ? (n + 3) / 4 * 4 : 0);       // dynamic; the row list is static on top
}
static_assert(peak_lds_bytes(PEAK_TILES[4][0], PEAK_TILES[4][1], DDPM3D_PEAK_MAX_RADIUS, DDPM3D_PEAK_MAX_RADIUS,
                             DDPM3D_PEAK_MAX_RADIUS, true) + PEAK_LDS_STATIC <= HALO_LDS_ALL,
              "the smallest tile of the largest footprint fits a CU's LDS");

// grid: x = tiles along W x tiles along H, y = tiles along D (strided: an extent may exceed a grid's y range),
// z = volume b.  A wave owns the TD outputs above one another at (y, lane): TD independent sums, so that TD (and
// with the +-k pair 2 TD) LDS reads are in flight before the first add waits.  Every output adds its taps in the order
// of the row list (dz, dy ascending), then dx = 0, -1, +1, -2, +2, ...  Six waves per SIMD is what the small tiles of a
// footprint along W alone can fill (21 KB of LDS a workgroup); the register allocator is held to it.
template <bool KEEP, int TD>
__global__ __launch_bounds__(HALO_THREADS) __attribute__((amdgpu_waves_per_eu(6)))
void sphere_mean_kernel(const float* __restrict__ vol, const uint8_t* __restrict__ keep, float* __restrict__ out,
                        const PeakArgs a) {
    extern __shared__ float lds[];
    __shared__ int s_rows[PEAK_SIDE * PEAK_SIDE];
    const HaloFrame f = halo_frame(TD, a.TH, a.r0, a.r1, a.rw, a.D, a.H, a.W);
    const auto [LW, LH, LD, slab, lane, wave, tiles_w, tiles_d, tx0, ty0, plane] = f;   // the compute loop's names
    const int64_t x = tx0 + lane;
    float* __restrict__ sx = lds;
    uint8_t* __restrict__ sk = reinterpret_cast<uint8_t*>(lds + (size_t)LD * slab);
    const int64_t base = (int64_t)blockIdx.z * a.D * plane;
    for (int i = threadIdx.x; i < a.n_rows; i += HALO_THREADS) s_rows[i] = a.rows[i];

    for (int tz = blockIdx.y; tz < tiles_d; tz += gridDim.y) {
        const int64_t tz0 = (int64_t)tz * TD;
        // stage with zeros outside the volume and where keep == 0; a word is the value and, with keep, its flag
        const int64_t gx0 = tx0 - a.rw + lane, gx1 = gx0 + 64;
        const bool x0_in = gx0 >= 0 && gx0 < a.W, x1_in = lane < 2 * a.rw && gx1 < a.W;
        struct Word { float v; uint8_t k; };
        halo_stage<Word>(
            f, 2 * a.rw,
            [&](int row, Word& w0, Word& w1) {
                const int64_t gz = tz0 - a.r0 + row / f.LH, gy = f.ty0 - a.r1 + row % f.LH;
                const bool row_in = (row < f.LD * f.LH) & (gz >= 0) & (gz < a.D) & (gy >= 0) & (gy < a.H);
                const int64_t at = gz * f.plane + gy * a.W;
                if (KEEP) {                                   // one test per word covers the value and its flag
                    w0 = w1 = Word{0.0f, 0};
                    if (row_in & x0_in) {
                        w0.v = vol[base + at + gx0];
                        w0.k = keep[at + gx0];
                    }
                    if (row_in & x1_in) {
                        w1.v = vol[base + at + gx1];
                        w1.k = keep[at + gx1];
                    }
                } else {
                    w0.v = row_in && x0_in ? vol[base + at + gx0] : 0.0f;
                    w1.v = row_in && x1_in ? vol[base + at + gx1] : 0.0f;
                }
            },
            [&](int at, const Word& w) {
                // with keep a select, not a product: an unkept NaN does not get in
                sx[at] = !KEEP || w.k ? w.v : 0.0f;
                if (KEEP) sk[at] = w.k ? 1 : 0;
            });
        __syncthreads();

        // the whole footprint of every voxel of the tile lies inside the volume: n is the tap count
        const bool inner = tz0 >= a.r0 && a.D - tz0 >= TD + a.r0 && ty0 >= a.r1 && a.H - ty0 >= a.TH + a.r1 &&
                           tx0 >= a.rw && a.W - tx0 >= HALO_TW + a.rw;
        for (int oy = wave; oy < a.TH; oy += HALO_THREADS / 64) {
            const int64_t y = ty0 + oy;
            if (y >= a.H) break;                              // the same for all lanes of the wave
            float acc[TD];
            int n[TD];
#pragma unroll
            for (int j = 0; j < TD; ++j) {
                acc[j] = -0.0f;                               // -0 + x = x for every x: one tap gives the voxel's own bits
                n[j] = 0;
            }
            int next = __builtin_amdgcn_readfirstlane(s_rows[0]);
            for (int i = 0; i < a.n_rows; ++i) {
                const int packed = next;
                // the next row's entry is on its way while this row's taps are read
                next = __builtin_amdgcn_readfirstlane(s_rows[i + 1 < a.n_rows ? i + 1 : i]);
                const int dz = (packed & 255) - a.r0, dy = ((packed >> 8) & 255) - a.r1, w = packed >> 16;
                // the row's centre tap for output j = 0; output j reads j planes further on
                const int at = ((a.r0 + dz) * LH + oy + a.r1 + dy) * LW + a.rw + lane;
#pragma unroll
                for (int j = 0; j < TD; ++j) {
                    acc[j] += sx[at + j * slab];
                    if (KEEP) n[j] += sk[at + j * slab];
                }
#pragma unroll
                for (int k = 1; k <= DDPM3D_PEAK_MAX_RADIUS; ++k) {
                    if (k > w) break;                         // the same for all lanes
#pragma unroll
                    for (int j = 0; j < TD; ++j) {
                        acc[j] += sx[at + j * slab - k];
                        acc[j] += sx[at + j * slab + k];
                        if (KEEP) n[j] += sk[at + j * slab - k] + sk[at + j * slab + k];
                    }
                }
                // without keep the count needs no taps: a row inside the volume adds its run clipped to the two W faces
                if (!KEEP && !inner && y + dy >= 0 && y + dy < a.H) {
                    const int64_t left = x < w ? x : w, right = a.W - 1 - x < w ? a.W - 1 - x : w;
                    const int run = (int)(left + right + 1);
#pragma unroll
                    for (int j = 0; j < TD; ++j) n[j] += (tz0 + j + dz >= 0 && tz0 + j + dz < a.D) ? run : 0;
                }
            }
            if (x < a.W) {
#pragma unroll
                for (int j = 0; j < TD; ++j) {
                    if (tz0 + j >= a.D) break;
                    const int cnt = (!KEEP && inner) ? a.taps : n[j];
                    out[base + (tz0 + j) * plane + y * a.W + x] = cnt > 0 ? acc[j] / (float)cnt : 0.0f;
                }
            }
        }
        __syncthreads();                                      // the next tile overwrites the LDS
    }
}

HaloPick peak_tile(int r0, int r1, int rw, bool keep) {
    return halo_pick(PEAK_TILES, PEAK_LDS_FOUR, PEAK_LDS_STATIC,
                     [=](int TD, int TH) { return peak_lds_bytes(TD, TH, r0, r1, rw, keep); });
}

template <bool KEEP, int TD>
constexpr auto peak_launch = halo_launch<sphere_mean_kernel<KEEP, TD>, const float*, const uint8_t*, float*, PeakArgs>;
template <bool KEEP>
constexpr auto peak_launch_td(int TD) {
    return TD == 8 ? peak_launch<KEEP, 8> : TD == 4 ? peak_launch<KEEP, 4> : TD == 2 ? peak_launch<KEEP, 2>
                                                                                       : peak_launch<KEEP, 1>;
}

}  // namespace

hipError_t ddpm3d_launch_sphere_mean(const float* vol, const uint8_t* keep, int B, int D, int H, int W, int r0, int r1,
                                     const int32_t* half_w, float* out, hipStream_t st) {
    PeakArgs a;
    a.D = D, a.H = H, a.W = W, a.r0 = r0, a.r1 = r1, a.rw = 0, a.taps = 0, a.n_rows = 0;
    for (int i = 0; i < (2 * r0 + 1) * (2 * r1 + 1); ++i) {
        const int w = half_w[i];
        if (w < 0) continue;
        a.rows[a.n_rows++] = (i / (2 * r1 + 1)) | (i % (2 * r1 + 1)) << 8 | w << 16;
        if (w > a.rw) a.rw = w;
        a.taps += 2 * w + 1;
    }
    for (int i = a.n_rows; i < PEAK_SIDE * PEAK_SIDE; ++i) a.rows[i] = 0;
    const HaloPick tile = peak_tile(r0, r1, a.rw, keep != nullptr);
    if (tile.lds_bytes == 0) return hipErrorInvalidValue;    // not reached for radii within DDPM3D_PEAK_MAX_RADIUS
    a.TD = tile.TD, a.TH = tile.TH;
    const auto launch = keep ? peak_launch_td<true>(a.TD) : peak_launch_td<false>(a.TD);
    return launch(halo_grid(B, D, H, W, a.TD, a.TH), tile.lds_bytes, PEAK_LDS_STATIC, st, vol, keep, out, a);
}
