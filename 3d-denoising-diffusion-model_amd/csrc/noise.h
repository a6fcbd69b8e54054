// Counter-based sampler noise: a standard normal as a pure function of
// (seed, stream, draw, voxel index), evaluated by the kernel that consumes it.  Philox4x32-10 (Salmon et al.,
// SC'11) gives four words per counter (index >> 2, draw, stream lo, stream hi) under the key (seed lo, seed hi);
// words (0, 1) make voxel lanes 0 and 1, words (2, 3) lanes 2 and 3, by Box-Muller on the precise device functions.
// The step kernels of ops.hip are templates on their noise source: TensorNoise reads the caller's tensor (the
// un-keyed entries, unchanged), KeyNoise evaluates the function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ddpm3d.h"

// ddpm3d_noise_key as the kernels take it (by value)
struct NoiseKeyDev {
    uint32_t k0, k1, draw;
    const int64_t* stream;
    const int32_t* origin;      // [N][3] or null
    int pd, ph, pw, Dc, Hc, Wc; // read only with an origin
};

static inline NoiseKeyDev noise_key_dev(const ddpm3d_noise_key& k) {
    NoiseKeyDev d;
    d.k0 = (uint32_t)(k.seed & 0xffffffffull);
    d.k1 = (uint32_t)(k.seed >> 32);
    d.draw = (uint32_t)k.draw;
    d.stream = k.stream;
    d.origin = k.origin;
    d.pd = k.patch[0]; d.ph = k.patch[1]; d.pw = k.patch[2];
    d.Dc = k.canvas[0]; d.Hc = k.canvas[1]; d.Wc = k.canvas[2];
    return d;
}

struct uint4w { uint32_t w[4]; };

__device__ __forceinline__ uint4w philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return uint4w{{c0, c1, c2, c3}};
}

// Two normals from two words.  u1 = fma(w_a, 2^-32, 2^-33) lies in (0, 1] (one rounding), u2 = w_b 2^-32; every
// operation rounds once, in this order, whichever kernel inlines it.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& even, float& odd) {
#pragma clang fp contract(off)
    const float u1 = fmaf((float)wa, 0x1p-32f, 0x1p-33f);
    const float u2 = (float)wb * 0x1p-32f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    even = r * c;
    odd = r * s;
}

// the normal of `index` (below 2^34) of one stream
__device__ __forceinline__ float noise_at(const NoiseKeyDev& k, uint32_t s_lo, uint32_t s_hi, uint64_t index) {
    const uint4w w = philox4x32_10((uint32_t)(index >> 2), k.draw, s_lo, s_hi, k.k0, k.k1);
    const bool high = (index & 2) != 0;
    float even, odd;
    box_muller(high ? w.w[2] : w.w[0], high ? w.w[3] : w.w[1], even, odd);
    return (index & 1) ? odd : even;
}

// ---- the step kernels' noise sources: src.sample(n) once per workgroup, then at(i, v) per voxel
// (i = n * voxels + v); ok() false = the sample's outputs are NaN-filled, nothing else is written
struct TensorNoise {
    const float* __restrict__ p;
    struct Sample {
        const float* __restrict__ p;
        __device__ __forceinline__ bool ok() const { return true; }
        __device__ __forceinline__ float at(size_t i, int) const { return p[i]; }
    };
    __device__ __forceinline__ bool present() const { return p != nullptr; }
    __device__ __forceinline__ Sample sample(int) const { return Sample{p}; }
};

struct KeyNoise {
    NoiseKeyDev k;
    struct Sample {
        NoiseKeyDev k;
        uint32_t s_lo, s_hi;
        int z0, y0, x0;
        bool inside;
        __device__ __forceinline__ bool ok() const { return inside; }
        __device__ __forceinline__ uint64_t index(int v) const {
            if (k.origin == nullptr) return (uint64_t)v;
            const int x = v % k.pw, zy = v / k.pw;
            const int y = zy % k.ph, z = zy / k.ph;
            return ((uint64_t)(z0 + z) * k.Hc + (uint64_t)(y0 + y)) * k.Wc + (uint64_t)(x0 + x);
        }
        __device__ __forceinline__ float at(size_t, int v) const { return noise_at(k, s_lo, s_hi, index(v)); }
    };
    __device__ __forceinline__ bool present() const { return true; }
    __device__ __forceinline__ Sample sample(int n) const {
        Sample s;
        s.k = k;
        const uint64_t id = (uint64_t)k.stream[n];
        s.s_lo = (uint32_t)id;
        s.s_hi = (uint32_t)(id >> 32);
        s.z0 = s.y0 = s.x0 = 0;
        s.inside = true;
        if (k.origin != nullptr) {
            s.z0 = k.origin[n * 3]; s.y0 = k.origin[n * 3 + 1]; s.x0 = k.origin[n * 3 + 2];
            // every voxel of the patch on the canvas (64-bit sums: an origin near INT_MAX cannot wrap)
            s.inside = s.z0 >= 0 && s.y0 >= 0 && s.x0 >= 0 && (int64_t)s.z0 + k.pd <= k.Dc &&
                       (int64_t)s.y0 + k.ph <= k.Hc && (int64_t)s.x0 + k.pw <= k.Wc;
        }
        return s;
    }
};

// noise.hip
hipError_t ddpm3d_launch_noise_fill(const ddpm3d_noise_key& key, int N, int voxels, float* out, hipStream_t st);
hipError_t ddpm3d_launch_noise_bits(const ddpm3d_noise_key& key, int N, int quads, uint32_t* out, hipStream_t st);
