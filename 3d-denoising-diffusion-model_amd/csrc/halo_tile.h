// The frame of the halo-tile kernels (peak.hip, nlm.hip; DESIGN.md 3.12 "The halo-tile frame"); none of their
// arithmetic.  A workgroup of four waves owns an output tile of TD x TH x 64 voxels, lane = x, and stages the tile plus
// a halo of (R0, R1, R2) voxels per side in dynamic LDS, so every LDS read of a wave is 64 consecutive words.  Tiles
// along D are walked with a strided blockIdx.y (an extent may exceed a grid's y range); a thread owns the TD outputs
// above one another.  (TD, TH) is picked on the host from a kernel's list of five against a small LDS budget (several
// workgroups per CU) and, failing that, the whole CU's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ops.h"

constexpr int HALO_THREADS = 256;
constexpr int HALO_TW = 64;                                   // one wave spans the tile along W
constexpr int HALO_STAGE_ROWS = 8;                            // rows a wave has in flight while staging
constexpr size_t HALO_LDS_ALL = 160 * 1024;                   // the LDS of a CU
constexpr size_t HALO_LDS_PLAIN = 64 * 1024;                  // what a launch may use without raising the kernel's limit

// words of the staged tile plus halo
constexpr size_t halo_words(int TD, int TH, int R0, int R1, int R2) {
    return (size_t)(TD + 2 * R0) * (TH + 2 * R1) * (HALO_TW + 2 * R2);
}

// tiles in a kernel's order of preference: the first whose dynamic bytes(TD, TH) plus the kernel's static bytes fit
// `small`, else the first that fits HALO_LDS_ALL; lds_bytes = 0 if none does
struct HaloPick { int TD, TH; size_t lds_bytes; };
template <class Bytes>
HaloPick halo_pick(const int (&tiles)[5][2], size_t small, size_t lds_static, Bytes bytes) {
    const size_t budgets[2] = {small, HALO_LDS_ALL};
    for (size_t budget : budgets) {
        for (const auto& t : tiles) {
            const size_t need = bytes(t[0], t[1]);
            if (need + lds_static <= budget) return {t[0], t[1], need};
        }
    }
    return {0, 0, 0};
}

// grid: x = tiles along W x tiles along H, y = tiles along D, z = volume b.  H * W <= 2^31 - 1, so the x extent fits;
// the y extent is capped and the kernel strides over the tiles along D
inline dim3 halo_grid(int B, int D, int H, int W, int TD, int TH) {
    const int64_t tiles_hw = (((int64_t)W + HALO_TW - 1) / HALO_TW) * (((int64_t)H + TH - 1) / TH);
    const int tiles_d = (int)(((int64_t)D + TD - 1) / TD);
    return dim3((unsigned)tiles_hw, (unsigned)(tiles_d < 65535 ? tiles_d : 65535), (unsigned)B);
}

// beyond HALO_LDS_PLAIN this instantiation's limit is raised to all a CU has, once per device and not per launch
template <auto Kernel, class... Args>
hipError_t halo_launch(dim3 grid, size_t lds_bytes, size_t lds_static, hipStream_t st, Args... args) {
    if (lds_bytes + lds_static > HALO_LDS_PLAIN) {
        static DynLdsOnce once = {};
        const hipError_t e = ddpm3d_allow_dynamic_lds(once, reinterpret_cast<const void*>(Kernel),
                                                      (int)(HALO_LDS_ALL - lds_static));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(Kernel, grid, dim3(HALO_THREADS), lds_bytes, st, args...);
    return hipGetLastError();
}

// what a workgroup knows before it walks its tiles: for (tz = blockIdx.y; tz < tiles_d; tz += gridDim.y)
struct HaloFrame {
    int LW, LH, LD, slab;                                     // the staged extents; slab = words per staged plane
    int lane, wave;
    int tiles_w, tiles_d;
    // 64-bit coordinates: an extent may be 2^31 - 1, and a tile or its halo reaches past it
    int64_t tx0, ty0, plane;
};
__device__ __forceinline__ HaloFrame halo_frame(int TD, int TH, int R0, int R1, int R2, int D, int H, int W) {
    HaloFrame f;
    f.LW = HALO_TW + 2 * R2, f.LH = TH + 2 * R1, f.LD = TD + 2 * R0;
    f.slab = f.LH * f.LW;
    f.lane = threadIdx.x & 63, f.wave = threadIdx.x >> 6;
    f.tiles_w = (int)(((int64_t)W + HALO_TW - 1) / HALO_TW);
    f.tiles_d = (int)(((int64_t)D + TD - 1) / TD);
    f.tx0 = (int64_t)(blockIdx.x % f.tiles_w) * HALO_TW;
    f.ty0 = (int64_t)(blockIdx.x / f.tiles_w) * TH;
    f.plane = (int64_t)H * W;
    return f;
}

// stage the LD x LH rows of LW = 64 + tail words: a wave takes HALO_STAGE_ROWS consecutive rows at a time, a lane the
// words lane and (the tail) lane + 64 of each.  load(row, w0, w1) reads both words of a row (row may lie past the last:
// the padding rule is the caller's, and so is what a word of type Word holds); store(at, w) writes one to LDS index at.
// The rows in flight live here, not in arrays that the two lambdas capture (those let the compiler wait on each load
// in turn); all loads of a batch are issued before the first is used.
template <class Word, class Load, class Store>
__device__ __forceinline__ void halo_stage(const HaloFrame& f, int tail, Load load, Store store) {
    for (int row0 = f.wave * HALO_STAGE_ROWS; row0 < f.LD * f.LH; row0 += HALO_THREADS / 64 * HALO_STAGE_ROWS) {
        Word w0[HALO_STAGE_ROWS], w1[HALO_STAGE_ROWS];
#pragma unroll
        for (int r = 0; r < HALO_STAGE_ROWS; ++r) load(row0 + r, w0[r], w1[r]);
#pragma unroll
        for (int r = 0; r < HALO_STAGE_ROWS; ++r) {
            const int row = row0 + r;
            if (row >= f.LD * f.LH) break;
            store(row * f.LW + f.lane, w0[r]);
            if (f.lane < tail) store(row * f.LW + 64 + f.lane, w1[r]);
        }
    }
}
