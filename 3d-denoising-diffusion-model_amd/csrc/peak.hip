// Sphere-mean map for SUVpeak (definitions in include/ddpm3d.h): out[b][v] = mean of vol[b] over the
// footprint voxels around v that lie inside the volume and are kept.  One dense pass.  A workgroup of four waves owns
// an output tile of TD x TH x 64 voxels, stages the tile plus its halo in LDS (zeros outside the volume and where
// keep == 0; with keep also one flag byte per voxel) and sums the footprint's row runs from there: lane = x, so every
// LDS read of a wave is 64 consecutive words.  The footprint travels in the kernel arguments as the list of its
// present rows (dz, dy, half-width), which a workgroup copies to LDS once, so each row's half-width is a scalar.  Taps
// are added in one order whatever the tile: the same bits on every run, and row b does not depend on B.  No atomics;
// plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int PEAK_THREADS = 256;
constexpr int PEAK_TW = 64;                                   // one wave spans the tile along W
constexpr int PEAK_SIDE = 2 * DDPM3D_PEAK_MAX_RADIUS + 1;
constexpr size_t PEAK_LDS_FOUR = 40 * 1024;                   // a tile this small leaves room for four workgroups per CU
constexpr int PEAK_STAGE_ROWS = 8;                            // rows a wave has in flight while staging
constexpr size_t PEAK_LDS_ALL = 160 * 1024;                   // the LDS of a CU
constexpr size_t PEAK_LDS_PLAIN = 64 * 1024;                  // what a launch may use without raising the kernel's limit
constexpr size_t PEAK_LDS_STATIC = sizeof(int) * PEAK_SIDE * PEAK_SIDE;   // the row list
// tiles in order of preference: the first that fits PEAK_LDS_FOUR, else the first that fits PEAK_LDS_ALL
constexpr int PEAK_TILES[5][2] = {{8, 8}, {4, 8}, {4, 4}, {2, 4}, {1, 4}};

struct PeakArgs {
    int D, H, W;
    int r0, r1, rw;                                           // rw = the largest half-width of the table
    int TD, TH;
    int taps;                                                 // the whole footprint's voxel count
    int n_rows;                                               // present rows, in the order dz, dy ascending
    int rows[PEAK_SIDE * PEAK_SIDE];                          // (dz + r0) | (dy + r1) << 8 | half-width << 16
};

constexpr size_t peak_lds_bytes(int TD, int TH, int r0, int r1, int rw, bool keep) {
    const size_t n = (size_t)(TD + 2 * r0) * (TH + 2 * r1) * (PEAK_TW + 2 * rw);
    return n * sizeof(float) + (keep ? (n + 3) / 4 * 4 : 0);       // dynamic; the row list is static on top
}
static_assert(peak_lds_bytes(PEAK_TILES[4][0], PEAK_TILES[4][1], DDPM3D_PEAK_MAX_RADIUS, DDPM3D_PEAK_MAX_RADIUS,
                             DDPM3D_PEAK_MAX_RADIUS, true) + PEAK_LDS_STATIC <= PEAK_LDS_ALL,
              "the smallest tile of the largest footprint fits a CU's LDS");

// grid: x = tiles along W x tiles along H, y = tiles along D (strided: an extent may exceed a grid's y range),
// z = volume b.  A wave owns the TD outputs above one another at (y, lane): TD independent sums, so that TD (and
// with the +-k pair 2 TD) LDS reads are in flight before the first add waits.  Every output adds its taps in the order
// of the row list (dz, dy ascending), then dx = 0, -1, +1, -2, +2, ...
template <bool KEEP, int TD>
__global__ __launch_bounds__(PEAK_THREADS) void sphere_mean_kernel(const float* __restrict__ vol,
                                                                   const uint8_t* __restrict__ keep,
                                                                   float* __restrict__ out, const PeakArgs a) {
    extern __shared__ float lds[];
    __shared__ int s_rows[PEAK_SIDE * PEAK_SIDE];
    const int LW = PEAK_TW + 2 * a.rw, LH = a.TH + 2 * a.r1, LD = TD + 2 * a.r0;
    const int slab = LH * LW;                                 // words per staged plane
    float* __restrict__ sx = lds;
    uint8_t* __restrict__ sk = reinterpret_cast<uint8_t*>(lds + (size_t)LD * slab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles_w = (int)(((int64_t)a.W + PEAK_TW - 1) / PEAK_TW);
    const int tiles_d = (int)(((int64_t)a.D + TD - 1) / TD);
    // 64-bit coordinates: an extent may be 2^31 - 1, and a tile or its halo reaches past it
    const int64_t tx0 = (int64_t)(blockIdx.x % tiles_w) * PEAK_TW;
    const int64_t ty0 = (int64_t)(blockIdx.x / tiles_w) * a.TH;
    const int64_t x = tx0 + lane;
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t base = (int64_t)blockIdx.z * a.D * plane;
    for (int i = threadIdx.x; i < a.n_rows; i += PEAK_THREADS) s_rows[i] = a.rows[i];

    for (int tz = blockIdx.y; tz < tiles_d; tz += gridDim.y) {
        const int64_t tz0 = (int64_t)tz * TD;
        // stage: a wave takes PEAK_STAGE_ROWS consecutive rows of the tile plus halo at a time, a lane the words lane
        // and (the tail of 2 rw words) lane + 64 of each; all loads of the batch are issued before the first is used
        const int64_t gx0 = tx0 - a.rw + lane, gx1 = gx0 + 64;
        const bool x0_in = gx0 >= 0 && gx0 < a.W, x1_in = lane < 2 * a.rw && gx1 < a.W;
        for (int row0 = wave * PEAK_STAGE_ROWS; row0 < LD * LH; row0 += PEAK_THREADS / 64 * PEAK_STAGE_ROWS) {
            float v0[PEAK_STAGE_ROWS], v1[PEAK_STAGE_ROWS];
            uint8_t k0[PEAK_STAGE_ROWS], k1[PEAK_STAGE_ROWS];
#pragma unroll
            for (int r = 0; r < PEAK_STAGE_ROWS; ++r) {
                const int row = row0 + r;
                const int64_t gz = tz0 - a.r0 + row / LH, gy = ty0 - a.r1 + row % LH;
                const bool row_in = row < LD * LH && gz >= 0 && gz < a.D && gy >= 0 && gy < a.H;
                const int64_t at = gz * plane + gy * a.W;
                v0[r] = row_in && x0_in ? vol[base + at + gx0] : 0.0f;
                v1[r] = row_in && x1_in ? vol[base + at + gx1] : 0.0f;
                if (KEEP) {
                    k0[r] = row_in && x0_in ? keep[at + gx0] : 0;
                    k1[r] = row_in && x1_in ? keep[at + gx1] : 0;
                }
            }
#pragma unroll
            for (int r = 0; r < PEAK_STAGE_ROWS; ++r) {
                const int row = row0 + r;
                if (row >= LD * LH) break;
                // with keep a select, not a product: an unkept NaN does not get in
                sx[row * LW + lane] = !KEEP || k0[r] ? v0[r] : 0.0f;
                if (KEEP) sk[row * LW + lane] = k0[r] ? 1 : 0;
                if (lane < 2 * a.rw) {
                    sx[row * LW + 64 + lane] = !KEEP || k1[r] ? v1[r] : 0.0f;
                    if (KEEP) sk[row * LW + 64 + lane] = k1[r] ? 1 : 0;
                }
            }
        }
        __syncthreads();

        // the whole footprint of every voxel of the tile lies inside the volume: n is the tap count
        const bool inner = tz0 >= a.r0 && a.D - tz0 >= TD + a.r0 && ty0 >= a.r1 && a.H - ty0 >= a.TH + a.r1 &&
                           tx0 >= a.rw && a.W - tx0 >= PEAK_TW + a.rw;
        for (int oy = wave; oy < a.TH; oy += PEAK_THREADS / 64) {
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

template <bool KEEP>
hipError_t peak_launch(const float* vol, const uint8_t* keep, float* out, const PeakArgs& a, dim3 grid, size_t lds_bytes,
                       hipStream_t st) {
    void (*fn)(const float*, const uint8_t*, float*, const PeakArgs) =
        a.TD == 8 ? sphere_mean_kernel<KEEP, 8> : a.TD == 4 ? sphere_mean_kernel<KEEP, 4>
        : a.TD == 2 ? sphere_mean_kernel<KEEP, 2> : sphere_mean_kernel<KEEP, 1>;
    if (lds_bytes + PEAK_LDS_STATIC > PEAK_LDS_PLAIN) {
        // raise this instantiation's limit to all a CU has, once per device (bit d of the mask), not per launch
        static std::atomic<unsigned long long> raised[4];
        std::atomic<unsigned long long>& mask = raised[a.TD == 8 ? 0 : a.TD == 4 ? 1 : a.TD == 2 ? 2 : 3];
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return e;
        const unsigned long long bit = device < 64 ? 1ull << device : 0;   // beyond 64 devices: set it every time
        if (!(mask.load(std::memory_order_acquire) & bit)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(PEAK_LDS_ALL - PEAK_LDS_STATIC));
            if (e != hipSuccess) return e;
            mask.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(fn, grid, dim3(PEAK_THREADS), lds_bytes, st, vol, keep, out, a);
    return hipGetLastError();
}

}  // namespace

void ddpm3d_sphere_mean_tile(int r0, int r1, int rw, bool keep, int* TD, int* TH, size_t* lds_bytes) {
    const size_t budgets[2] = {PEAK_LDS_FOUR, PEAK_LDS_ALL};
    for (size_t budget : budgets) {
        for (const auto& t : PEAK_TILES) {
            const size_t need = peak_lds_bytes(t[0], t[1], r0, r1, rw, keep);
            if (need + PEAK_LDS_STATIC <= budget) {
                *TD = t[0];
                *TH = t[1];
                *lds_bytes = need;
                return;
            }
        }
    }
    *TD = *TH = 0;                                            // not reached for radii within DDPM3D_PEAK_MAX_RADIUS
    *lds_bytes = 0;
}

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
    size_t lds_bytes = 0;
    ddpm3d_sphere_mean_tile(r0, r1, a.rw, keep != nullptr, &a.TD, &a.TH, &lds_bytes);
    if (lds_bytes == 0) return hipErrorInvalidValue;
    // H * W <= 2^31 - 1, so the x extent fits; the y extent is capped and the kernel strides over the tiles along D
    const int64_t tiles_hw = (((int64_t)W + PEAK_TW - 1) / PEAK_TW) * (((int64_t)H + a.TH - 1) / a.TH);
    const int tiles_d = (int)(((int64_t)D + a.TD - 1) / a.TD);
    const dim3 grid((unsigned)tiles_hw, (unsigned)(tiles_d < 65535 ? tiles_d : 65535), (unsigned)B);
    return keep ? peak_launch<true>(vol, keep, out, a, grid, lds_bytes, st)
                : peak_launch<false>(vol, keep, out, a, grid, lds_bytes, st);
}
