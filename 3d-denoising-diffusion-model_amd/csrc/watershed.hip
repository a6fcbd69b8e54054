// Watershed basins of a height volume inside labelled components, and the saddle graph between them (DESIGN.md 3.24;
// the definition is in include/ddpm3d.h).  Foreground: labels > 0 and a height that is no NaN.  Neighbours: adjacent
// under the connectivity, both foreground, same label.  Order: key(v) = (height[v], -v).
//   ddpm3d_basins         clear of the 16-byte accumulator, then
//     parent    a thread per voxel writes the voxel of greatest key among itself and its neighbours into peaks[v]
//     resolve   a thread per voxel walks the parents from peaks[v] to a slot that holds its own index (a peak) and
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

namespace {

constexpr int WS_THREADS = 256;
constexpr unsigned long long WS_EMPTY = ~0ull;            // no pair: basins are indices >= 0

struct Dims {
    int D, H, W;
};

// the accumulator in the workspace: both entries clear it first and copy it to status last
struct Acc {
    unsigned long long count;                             // peaks, or records needed
    int32_t flag;                                         // a loop hit its cap
    int32_t pad;
};
static_assert(sizeof(Acc) == 16, "ddpm3d_watershed_workspace_bytes");

// the neighbours with at most ORDER non-zero components; FORWARD: only those that follow the voxel in raster order,
// so that every unordered pair of voxels is looked at once (3, 9 or 13 directions)
template <int ORDER, bool FORWARD, typename F>
__device__ __forceinline__ void for_neighbours(F&& f) {
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int nz = (dz != 0) + (dy != 0) + (dx != 0);
                const bool forward = dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)));
                if (nz >= 1 && nz <= ORDER && (!FORWARD || forward)) f(dz, dy, dx);
            }
}

__device__ __forceinline__ int load_slot(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------- parent
template <int ORDER>
__global__ __launch_bounds__(WS_THREADS) void ws_parent_kernel(const float* __restrict__ height,
                                                               const int32_t* __restrict__ labels, Dims g, int n,
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
    const int x = v % g.W, y = v / g.W % g.H, z = v / g.W / g.H;
    int best = v;
    float bh = h;
    for_neighbours<ORDER, false>([&](int dz, int dy, int dx) {
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

// ---------------------------------------------------------------------------------------------------- resolve
// Slot v holds parent(v) at first and is written once more, by thread v alone, with the peak of v's chain.  Both are
// ancestors of v (or v), so whatever a walker reads in a slot lies further up the same chain: races change the path,
// never the end.  key(parent(u)) > key(u) unless parent(u) == u, so a chain has at most n links and the cap n is out
// of reach; an index outside [0, n) cannot have been written here and stops the walk with the flag set.
__global__ __launch_bounds__(WS_THREADS) void ws_resolve_kernel(int n, int32_t* peaks, Acc* __restrict__ acc) {
    __shared__ int wave_count[WS_THREADS / 64];
    const int64_t v64 = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x;
    int overrun = 0, mine = 0;
    if (v64 < n) {
        const int v = (int)v64;
        const int p = peaks[v];                           // only this thread writes slot v in this launch
        if (p == v) {
            mine = 1;
        } else if (p >= 0) {
            int at = p;
            bool done = false;
            for (int it = 0; it < n; ++it) {
                if ((unsigned)at >= (unsigned)n) break;
                const int up = load_slot(peaks + at);
                if (up == at) {
                    done = true;
                    break;
                }
                at = up;
            }
            if (!done) overrun = 1;
            else if (at != p) __hip_atomic_store(peaks + v, at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
    overrun = __syncthreads_or(overrun);
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < WS_THREADS / 64; ++w) total += wave_count[w];
        if (total) atomicAdd(&acc->count, (unsigned long long)total);
        if (overrun) atomicOr(&acc->flag, 1);
    }
}

__global__ void ws_finish_kernel(const Acc* __restrict__ acc, int32_t* __restrict__ status) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        status[0] = acc->flag ? 1 : 0;
        status[1] = acc->count > (unsigned long long)INT_MAX ? INT_MAX : (int32_t)acc->count;
    }
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
                                                               const int32_t* __restrict__ peaks, Dims g, int n,
                                                               int cap, int32_t* __restrict__ pairs,
                                                               float* __restrict__ saddle, Acc* __restrict__ acc) {
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
        const int x = v % g.W, y = v / g.W % g.H, z = v / g.W / g.H;
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
        if (overrun) atomicOr(&acc->flag, 1);
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
hipError_t launch_basins(const float* height, const int32_t* labels, Dims g, int n, int32_t* peaks, Acc* acc,
                         int32_t* status, hipStream_t st) {
    const unsigned blocks = (unsigned)(((int64_t)n + WS_THREADS - 1) / WS_THREADS);
    hipError_t e = hipMemsetAsync(acc, 0, sizeof(Acc), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_parent_kernel<ORDER>, dim3(blocks), dim3(WS_THREADS), 0, st, height, labels, g, n, peaks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_resolve_kernel, dim3(blocks), dim3(WS_THREADS), 0, st, n, peaks, acc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_finish_kernel, dim3(1), dim3(64), 0, st, acc, status);
    return hipGetLastError();
}

template <int ORDER>
hipError_t launch_saddles(const float* height, const int32_t* labels, const int32_t* peaks, Dims g, int n, int cap,
                          int32_t* pairs, float* saddle, Acc* acc, int32_t* status, hipStream_t st) {
    const unsigned blocks = (unsigned)(((int64_t)n + WS_THREADS - 1) / WS_THREADS);
    hipError_t e = hipMemsetAsync(acc, 0, sizeof(Acc), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_saddle_kernel<ORDER>, dim3(blocks), dim3(WS_THREADS), 0, st, height, labels, peaks, g, n,
                       cap, pairs, saddle, acc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ws_finish_kernel, dim3(1), dim3(64), 0, st, acc, status);
    return hipGetLastError();
}

}  // namespace

size_t ddpm3d_watershed_workspace_bytes() { return sizeof(Acc); }

hipError_t ddpm3d_launch_basins(const float* height, const int32_t* labels, int connectivity, int D, int H, int W,
                                int32_t* peaks, void* ws, int32_t* status, hipStream_t st) {
    const Dims g = {D, H, W};
    const int n = (int)((int64_t)D * H * W);
    if (connectivity == 6) return launch_basins<1>(height, labels, g, n, peaks, (Acc*)ws, status, st);
    if (connectivity == 18) return launch_basins<2>(height, labels, g, n, peaks, (Acc*)ws, status, st);
    return launch_basins<3>(height, labels, g, n, peaks, (Acc*)ws, status, st);
}

hipError_t ddpm3d_launch_basin_saddles(const float* height, const int32_t* labels, const int32_t* peaks,
                                       int connectivity, int D, int H, int W, int cap, int32_t* pairs, float* saddle,
                                       void* ws, int32_t* status, hipStream_t st) {
    const Dims g = {D, H, W};
    const int n = (int)((int64_t)D * H * W);
    if (connectivity == 6)
        return launch_saddles<1>(height, labels, peaks, g, n, cap, pairs, saddle, (Acc*)ws, status, st);
    if (connectivity == 18)
        return launch_saddles<2>(height, labels, peaks, g, n, cap, pairs, saddle, (Acc*)ws, status, st);
    return launch_saddles<3>(height, labels, peaks, g, n, cap, pairs, saddle, (Acc*)ws, status, st);
}
