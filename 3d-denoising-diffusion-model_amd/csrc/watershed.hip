// Watershed basins of a height volume inside labelled components, and the saddle graph between them (DESIGN.md 3.24;
// the definition is in include/ddpm3d.h).  Foreground: labels > 0 and a height that is no NaN.  Neighbours: adjacent
// under the connectivity, both foreground, same label.  Order: key(v) = (height[v], -v).
// The neighbours, the walk, flatten, finish and the 16-byte status accumulator are voxel_forest.h's.
//   ddpm3d_basins         clear of the accumulator, then
//     parent    a thread per voxel writes the voxel of greatest key among itself and its neighbours into peaks[v]:
//               key(parent(v)) > key(v) unless parent(v) == v, the order the shared walk needs
//     flatten   a thread per voxel walks the parents from peaks[v] to a slot that holds its own index (a peak) and
//               stores that: in place, so later walkers find shorter chains; peaks are counted per workgroup
//     finish    one thread copies the accumulator (cap flag, count) into status
//   ddpm3d_basin_saddles  clear, then
//     saddles   a thread per voxel looks at its 3, 9 or 13 forward neighbours; the pairs whose basins differ are
//               reduced per workgroup in an LDS hash table (one slot per pair, maximum of min(height, height)); the
//               table's slots get consecutive record numbers from one 64-bit atomicAdd per workgroup
//     finish
// No value read from height, labels or a caller's peaks is ever an address: they are compared and copied.  The only
// indices followed are the parents written here, and the walk checks each against the voxel count before it reads.
// No workgroup waits for another; every loop has a cap that a correct run cannot reach and that sets the flag.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "voxel_forest.h"

namespace {

constexpr int WS_THREADS = 256;
constexpr unsigned long long WS_EMPTY = ~0ull;            // no pair: basins are indices >= 0

// ---------------------------------------------------------------------------------------------------- parent
template <int ORDER>
__global__ __launch_bounds__(WS_THREADS) void ws_parent_kernel(const float* __restrict__ height,
                                                               const int32_t* __restrict__ labels, Extents g, int n,
                                                               int32_t* __restrict__ peaks) {
    const int64_t v64 = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x;
    if (v64 >= n) return;
    const int v = (int)v64;
    const int32_t l = labels[v];
    const float h = height[v];
    if (!(l > 0) || h != h) {
        peaks[v] = -1;
        return;
    }
    const Voxel at = voxel_of(g, v);
    const int z = at.z, y = at.y, x = at.x;
    int best = v;
    float bh = h;
    for_neighbours<ORDER>([&](int dz, int dy, int dx) {
        const int nz = z + dz, ny = y + dy, nx = x + dx;
        if (nz < 0 || nz >= g.D || ny < 0 || ny >= g.H || nx < 0 || nx >= g.W) return;
        const int u = v + (dz * g.H + dy) * g.W + dx;     // inside the volume: no overflow
        const float hu = height[u];
        if (labels[u] != l || hu != hu) return;
        if (hu > bh || (hu == bh && u < best)) {
            best = u;
            bh = hu;
        }
    });
    peaks[v] = best;
}

// ---------------------------------------------------------------------------------------------------- saddles
// fp32 without NaN <-> unsigned in the same order; 0 is below every value
__device__ __forceinline__ unsigned ordered(float f) {
    const unsigned b = __float_as_uint(f);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float unordered(unsigned o) {
    return __uint_as_float(o & 0x80000000u ? o & 0x7fffffffu : ~o);
}

template <int ORDER>
struct SaddleTable {
    static constexpr int DIRS = ORDER == 1 ? 3 : ORDER == 2 ? 9 : 13;
    // a power of two that holds every pair a workgroup can see, so an insertion always finds its slot or a free one
    static constexpr int SLOTS = ORDER == 1 ? 1024 : 4096;
    static constexpr int PER = SLOTS / WS_THREADS;
    static_assert(SLOTS >= DIRS * WS_THREADS && SLOTS * 12 <= 48 * 1024, "the table fits the pairs and 48 KiB of LDS");
};

template <int ORDER>
__global__ __launch_bounds__(WS_THREADS) void ws_saddle_kernel(const float* __restrict__ height,
                                                               const int32_t* __restrict__ labels,
                                                               const int32_t* __restrict__ peaks, Extents g, int n,
                                                               int cap, int32_t* __restrict__ pairs,
                                                               float* __restrict__ saddle,
                                                               ForestStatus* __restrict__ acc) {
    using T = SaddleTable<ORDER>;
    __shared__ unsigned long long keys[T::SLOTS];
    __shared__ unsigned vals[T::SLOTS];
    __shared__ int wave_total[WS_THREADS / 64];
    __shared__ long long base;
    const int tid = threadIdx.x;
    const int64_t v64 = (int64_t)blockIdx.x * WS_THREADS + tid;

    // every differing pair (a < b, min of the two heights) between this thread's voxel and its forward neighbours
    auto scan = [&](auto&& emit) {
        if (v64 >= n) return;
        const int v = (int)v64;
        const int32_t l = labels[v];
        const float h = height[v];
        if (!(l > 0) || h != h) return;
        const int32_t pv = peaks[v];
        const Voxel at = voxel_of(g, v);
        const int z = at.z, y = at.y, x = at.x;
        for_neighbours<ORDER, true>([&](int dz, int dy, int dx) {
            const int nz = z + dz, ny = y + dy, nx = x + dx;
            if (nz >= g.D || ny < 0 || ny >= g.H || nx < 0 || nx >= g.W) return;     // forward: nz >= z
            const int u = v + (dz * g.H + dy) * g.W + dx;
            const float hu = height[u];
            if (labels[u] != l || hu != hu) return;
            const int32_t pu = peaks[u];
            if (pu == pv) return;
            emit(pu < pv ? pu : pv, pu < pv ? pv : pu, hu < h ? hu : h);
        });
    };

    int any = 0;
    scan([&](int32_t, int32_t, float) { any = 1; });
    if (!__syncthreads_or(any)) return;                   // the whole workgroup lies inside basins: nothing to reduce

    for (int s = tid; s < T::SLOTS; s += WS_THREADS) {
        keys[s] = WS_EMPTY;
        vals[s] = 0;
    }
    __syncthreads();

    int overrun = 0;
    scan([&](int32_t a, int32_t b, float s) {
        const unsigned long long key = ((unsigned long long)(uint32_t)a << 32) | (uint32_t)b;
        unsigned slot = (((uint32_t)a * 0x9E3779B1u) ^ ((uint32_t)b * 0x85EBCA77u)) >> 16 & (T::SLOTS - 1);
        for (int it = 0; it < T::SLOTS; ++it) {           // at most DIRS * WS_THREADS <= SLOTS keys: a slot is found
            const unsigned long long old = atomicCAS(&keys[slot], WS_EMPTY, key);
            if (old == WS_EMPTY || old == key) {
                atomicMax(&vals[slot], ordered(s));
                return;
            }
            slot = (slot + 1) & (T::SLOTS - 1);
        }
        overrun = 1;
    });
    __syncthreads();

    // number the occupied slots: thread t owns slots [t * PER, (t + 1) * PER)
    int mine = 0;
#pragma unroll
    for (int j = 0; j < T::PER; ++j) mine += keys[tid * T::PER + j] != WS_EMPTY;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if ((tid & 63) >= o) incl += up;
    }
    if ((tid & 63) == 63) wave_total[tid >> 6] = incl;
    overrun = __syncthreads_or(overrun);
    int before = incl - mine;
    for (int w = 0; w < (tid >> 6); ++w) before += wave_total[w];
    if (tid == WS_THREADS - 1) {
        base = (long long)atomicAdd(&acc->count, (unsigned long long)(before + mine));
        if (overrun) flag_overrun(acc);
    }
    __syncthreads();
    int64_t at = base + before;
#pragma unroll
    for (int j = 0; j < T::PER; ++j) {
        const unsigned long long key = keys[tid * T::PER + j];
        if (key == WS_EMPTY) continue;
        if (at < cap) {                                   // records beyond the capacity are counted, never written
            pairs[2 * at] = (int32_t)(key >> 32);
            pairs[2 * at + 1] = (int32_t)(key & 0xffffffffu);
            saddle[at] = unordered(vals[tid * T::PER + j]);
        }
        ++at;
    }
}

template <int ORDER>
hipError_t launch_basins(const float* height, const int32_t* labels, Extents g, int32_t* peaks, ForestStatus* acc,
                         int32_t* status, hipStream_t st) {
    const int n = (int)((int64_t)g.D * g.H * g.W);
    const unsigned blocks = (unsigned)(((int64_t)n + WS_THREADS - 1) / WS_THREADS);
    hipError_t e = forest_clear(acc, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_parent_kernel<ORDER>, dim3(blocks), dim3(WS_THREADS), 0, st, height, labels, g, n, peaks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return forest_flatten_and_finish<1>(n, peaks, acc, nullptr, status, st);
}

template <int ORDER>
hipError_t launch_saddles(const float* height, const int32_t* labels, const int32_t* peaks, Extents g, int cap,
                          int32_t* pairs, float* saddle, ForestStatus* acc, int32_t* status, hipStream_t st) {
    const int n = (int)((int64_t)g.D * g.H * g.W);
    const unsigned blocks = (unsigned)(((int64_t)n + WS_THREADS - 1) / WS_THREADS);
    hipError_t e = forest_clear(acc, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_saddle_kernel<ORDER>, dim3(blocks), dim3(WS_THREADS), 0, st, height, labels, peaks, g, n,
                       cap, pairs, saddle, acc);
    e = hipGetLastError();
    return e != hipSuccess ? e : forest_finish(acc, nullptr, 0, status, st);
}

}  // namespace

size_t ddpm3d_watershed_workspace_bytes() { return sizeof(ForestStatus); }

hipError_t ddpm3d_launch_basins(const float* height, const int32_t* labels, int connectivity, int D, int H, int W,
                                int32_t* peaks, void* ws, int32_t* status, hipStream_t st) {
    return with_order(connectivity, [&](auto order) {
        return launch_basins<decltype(order)::value>(height, labels, {D, H, W}, peaks, (ForestStatus*)ws, status, st);
    });
}

hipError_t ddpm3d_launch_basin_saddles(const float* height, const int32_t* labels, const int32_t* peaks,
                                       int connectivity, int D, int H, int W, int cap, int32_t* pairs, float* saddle,
                                       void* ws, int32_t* status, hipStream_t st) {
    return with_order(connectivity, [&](auto order) {
        return launch_saddles<decltype(order)::value>(height, labels, peaks, {D, H, W}, cap, pairs, saddle,
                                                      (ForestStatus*)ws, status, st);
    });
}
