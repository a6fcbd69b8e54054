// Exact squared Euclidean distance transform on anisotropic voxels (definition and error bound in
// include/ddpm3d.h): three separable passes over K volumes [D][H][W], the last two in place on the output.
//   pass W: a wave owns a row.  It ballots the background of 64 voxels at a time: the nearest background voxel to the
//           left is the highest set bit at or below the lane, or the carry of the chunks before; the distances to the
//           left wait in LDS while a second sweep, from the right, finds the other side.  Loads and stores are 64
//           neighbouring voxels of one row.
//   pass H, pass D: a workgroup stages whole lines of DDPM3D_EDT_COLUMNS neighbouring columns in LDS (64 contiguous
//           bytes per line position), every lane owns outputs of one column and scans the line outward from its own
//           position, stopping once the squared offset alone reaches the best so far, and the workgroup writes its own
//           columns back: nothing else reads them, so the pass needs no second volume.
// For pass D the H x W plane is one row of H * W columns.  No atomics; a minimum over a fixed set, so the bits do not
// depend on the launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int EDT_THREADS = 256;                        // four waves
constexpr int EDT_WAVES = EDT_THREADS / 64;
constexpr int EDT_C = DDPM3D_EDT_COLUMNS;
constexpr int EDT_LANES_Y = EDT_THREADS / EDT_C;        // line positions a workgroup covers per sweep
constexpr int EDT_STEPS = 4;                            // offsets of the scan between two tests of its stopping rule
constexpr int EDT_NONE = 0x3fffffff;                    // "no background on this side"; 2 * EDT_NONE fits an int

static_assert(EDT_THREADS % EDT_C == 0, "a sweep covers whole line positions");
static_assert(DDPM3D_EDT_MAX_EXTENT * EDT_C * 4 <= 64 * 1024, "a group of lines fits the 64 KiB a launch may ask for");
static_assert(DDPM3D_EDT_MAX_EXTENT % 64 == 0, "pass W walks whole chunks of its LDS row");

// rows = K * D * H rows of W voxels; out[x] = (sw * n)^2, n the count of voxels to the row's nearest background voxel
__global__ __launch_bounds__(EDT_THREADS) void edt_row_kernel(const uint8_t* __restrict__ mask,
                                                              float* __restrict__ out, int64_t rows, int W,
                                                              int invert, float sw) {
    __shared__ int left[EDT_WAVES][DDPM3D_EDT_MAX_EXTENT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * EDT_WAVES + wave;
    if (row >= rows) return;                            // whole waves leave; no barrier follows
    const uint8_t* __restrict__ m = mask + row * W;
    float* __restrict__ o = out + row * W;
    const int chunks = (W + 63) >> 6;
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);    // bits 0..lane
    const uint64_t from = ~0ull << lane;                                // bits lane..63
    int carry = -EDT_NONE;                              // the last background voxel of the chunks before
    for (int c = 0; c < chunks; ++c) {
        const int x = c * 64 + lane;
        const bool bg = x < W && ((m[x] != 0) == (invert != 0));
        const uint64_t b = __ballot(bg);
        const uint64_t mine = b & upto;
        const int prev = mine ? c * 64 + 63 - __clzll((long long)mine) : carry;
        left[wave][x] = x - prev;                       // x < chunks * 64 <= DDPM3D_EDT_MAX_EXTENT
        if (b) carry = c * 64 + 63 - __clzll((long long)b);
    }
    carry = EDT_NONE;                                   // the first background voxel of the chunks after
    for (int c = chunks - 1; c >= 0; --c) {
        const int x = c * 64 + lane;
        const bool bg = x < W && ((m[x] != 0) == (invert != 0));
        const uint64_t b = __ballot(bg);
        const uint64_t mine = b & from;
        const int next = mine ? c * 64 + __ffsll((long long)mine) - 1 : carry;
        const int n = min(left[wave][x], next - x);     // this lane wrote left[wave][x] itself
        if (x < W) {
            const float t = sw * (float)n;
            o[x] = n >= EDT_NONE - DDPM3D_EDT_MAX_EXTENT ? __builtin_inff() : t * t;
        }
        if (b) carry = c * 64 + __ffsll((long long)b) - 1;
    }
}

// `outer` slabs of L lines of P columns: element (o, y, p) at o * L * P + y * P + p.  A workgroup takes EDT_C
// neighbouring columns of one slab: f(y) <- min over y' of fmaf(a, a, f(y')), a = s * (float)(y - y').
__global__ __launch_bounds__(EDT_THREADS) void edt_line_kernel(float* __restrict__ f, int L, int64_t P, int groups,
                                                               float s) {
    extern __shared__ float line[];                     // [L][EDT_C]
    const int64_t slab = blockIdx.x / groups;
    const int64_t p0 = (int64_t)(blockIdx.x % groups) * EDT_C;
    const int c = threadIdx.x % EDT_C, y0 = threadIdx.x / EDT_C;
    const bool live = p0 + c < P;
    float* __restrict__ col = f + slab * L * P + p0 + c;
    for (int y = y0; y < L; y += EDT_LANES_Y) line[y * EDT_C + c] = live ? col[(int64_t)y * P] : 0.0f;
    __syncthreads();
    if (!live) return;                                  // no barrier follows
    for (int y = y0; y < L; y += EDT_LANES_Y) {
        float best = line[y * EDT_C + c];
        // EDT_STEPS offsets per test: the candidates a later test would have cut cannot be strictly smaller, so the
        // minimum keeps its bits, and their LDS reads are in flight together
        for (int k0 = 1; k0 < L; k0 += EDT_STEPS) {
            const float a0 = s * (float)k0;
            if (a0 * a0 >= best) break;                 // fmaf(a, a, f) >= a * a rounded: nothing farther can win
            float cand[2 * EDT_STEPS];
#pragma unroll
            for (int j = 0; j < EDT_STEPS; ++j) {
                const int k = k0 + j;                   // k >= L fails both range tests
                const float a = s * (float)k;
                cand[2 * j] = y - k >= 0 ? fmaf(a, a, line[(y - k) * EDT_C + c]) : __builtin_inff();
                cand[2 * j + 1] = y + k < L ? fmaf(a, a, line[(y + k) * EDT_C + c]) : __builtin_inff();
            }
#pragma unroll
            for (int j = 0; j < 2 * EDT_STEPS; ++j) best = fminf(best, cand[j]);
        }
        col[(int64_t)y * P] = best;
    }
}

}  // namespace

hipError_t ddpm3d_launch_distance_sq(const uint8_t* mask, int K, int D, int H, int W, int invert, const float s[3],
                                     float* out, hipStream_t st) {
    const int64_t rows = (int64_t)K * D * H;
    const int64_t row_blocks = (rows + EDT_WAVES - 1) / EDT_WAVES;
    const int64_t groups_h = (W + EDT_C - 1) / EDT_C, blocks_h = (int64_t)K * D * groups_h;
    const int64_t plane = (int64_t)H * W;
    const int64_t groups_d = (plane + EDT_C - 1) / EDT_C, blocks_d = (int64_t)K * groups_d;
    if (row_blocks > 0x7fffffff || blocks_h > 0x7fffffff || blocks_d > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)row_blocks), dim3(EDT_THREADS), 0, st, mask, out, rows, W,
                       invert, s[2]);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (H > 1) {                                        // a line of one voxel is its own minimum
        hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)blocks_h), dim3(EDT_THREADS),
                           (size_t)H * EDT_C * sizeof(float), st, out, H, (int64_t)W, (int)groups_h, s[1]);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (D > 1) {
        hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)blocks_d), dim3(EDT_THREADS),
                           (size_t)D * EDT_C * sizeof(float), st, out, D, plane, (int)groups_d, s[0]);
        e = hipGetLastError();
    }
    return e;
}
