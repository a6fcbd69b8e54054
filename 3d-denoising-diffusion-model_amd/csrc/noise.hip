// ddpm3d_noise_fill / ddpm3d_noise_bits: the keyed noise function of noise.h written out -- the x_T of a keyed loop,
// and the bridge on which the keyed step kernels (ops.hip) are tested against the un-keyed ones.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "noise.h"

// one grid row per sample, at most 1024 workgroups striding over its items (the step kernels' convention)
static dim3 noise_grid(int N, int items) {
    int bx = (items + 255) / 256;
    if (bx > 1024) bx = 1024;
    return dim3(bx, N);
}

// Without a geometry: one thread per counter, i.e. one Philox call and two Box-Muller pairs for indices
// 4q .. 4q + 3.  Rows start at n * voxels, which is 16-byte aligned only by chance: four 4-byte stores.
__global__ __launch_bounds__(256) void noise_fill_quad_kernel(NoiseKeyDev k, int voxels, float* __restrict__ out) {
    const int n = blockIdx.y;
    const uint64_t id = (uint64_t)k.stream[n];
    const uint32_t s_lo = (uint32_t)id, s_hi = (uint32_t)(id >> 32);
    const int quads = (int)(((int64_t)voxels + 3) >> 2);
    float* row = out + (size_t)n * voxels;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        const uint4w w = philox4x32_10((uint32_t)q, k.draw, s_lo, s_hi, k.k0, k.k1);
        float z[4];
        box_muller(w.w[0], w.w[1], z[0], z[1]);
        box_muller(w.w[2], w.w[3], z[2], z[3]);
        const int64_t v0 = (int64_t)q * 4;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (v0 + l < voxels) row[v0 + l] = z[l];
    }
}

// With a geometry: the per-voxel form, exactly what a keyed step kernel evaluates.  A patch that leaves the canvas
// is NaN-filled.
__global__ __launch_bounds__(256) void noise_fill_voxel_kernel(KeyNoise src, int voxels, float* __restrict__ out) {
    const int n = blockIdx.y;
    const KeyNoise::Sample ns = src.sample(n);
    const bool ok = ns.ok();
    const float nan = __builtin_nanf("");
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += gridDim.x * blockDim.x) {
        const size_t i = (size_t)n * voxels + v;
        out[i] = ok ? ns.at(i, v) : nan;
    }
}

// the raw words of counters q = 0 .. quads - 1: out[n][q][4]
__global__ __launch_bounds__(256) void noise_bits_kernel(NoiseKeyDev k, int quads, uint32_t* __restrict__ out) {
    const int n = blockIdx.y;
    const uint64_t id = (uint64_t)k.stream[n];
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        const uint4w w = philox4x32_10((uint32_t)q, k.draw, (uint32_t)id, (uint32_t)(id >> 32), k.k0, k.k1);
        uint32_t* o = out + ((size_t)n * quads + q) * 4;
#pragma unroll
        for (int l = 0; l < 4; ++l) o[l] = w.w[l];
    }
}

hipError_t ddpm3d_launch_noise_fill(const ddpm3d_noise_key& key, int N, int voxels, float* out, hipStream_t st) {
    const NoiseKeyDev k = noise_key_dev(key);
    if (key.origin == nullptr)
        hipLaunchKernelGGL(noise_fill_quad_kernel, noise_grid(N, (int)(((int64_t)voxels + 3) >> 2)), dim3(256), 0, st,
                           k, voxels, out);
    else
        hipLaunchKernelGGL(noise_fill_voxel_kernel, noise_grid(N, voxels), dim3(256), 0, st, KeyNoise{k}, voxels, out);
    return hipGetLastError();
}

hipError_t ddpm3d_launch_noise_bits(const ddpm3d_noise_key& key, int N, int quads, uint32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(noise_bits_kernel, noise_grid(N, quads), dim3(256), 0, st, noise_key_dev(key), quads, out);
    return hipGetLastError();
}
