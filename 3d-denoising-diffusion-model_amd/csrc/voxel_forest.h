// The frame of the graph passes over a voxel volume: connected components (ccl.hip) and watershed
// basins (watershed.hip).  Both build a forest in an int32 volume -- slot v holds the index of v's parent, its own
// index at a root, -1 on the background -- while other workgroups rewrite slots, and both report through
// status[2] = {a loop hit its cap, a count}.  Here: the extents and the neighbours of a connectivity, the slot
// access, the one chain walk, the flatten kernel that replaces every slot by its root, and the status accumulator.
// Integer atomics only, so status carries the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <type_traits>

namespace {

constexpr int FOREST_THREADS = 256;

struct Extents {
    int D, H, W;
};
struct Voxel {
    int z, y, x;
};
__device__ __forceinline__ Voxel voxel_of(const Extents& g, int v) { return {v / g.W / g.H, v / g.W % g.H, v % g.W}; }

// The neighbours with at most ORDER non-zero components (6, 18 or 26 of them); FORWARD: only those that follow the
// voxel in raster order, so that every unordered pair of voxels is looked at once (3, 9 or 13 directions).
template <int ORDER, bool FORWARD = false, typename F>
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

// connectivity 6 / 18 / 26 (the caller has checked it) -> f(std::integral_constant<int, ORDER>)
template <typename F>
hipError_t with_order(int connectivity, F&& f) {
    if (connectivity == 6) return f(std::integral_constant<int, 1>{});
    if (connectivity == 18) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 3>{});
}

__device__ __forceinline__ int load_slot(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_slot(int32_t* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Follows parent slots from `at` to a slot that holds its own index and returns that root.  The caller's forest has a
// strict order in which every slot that is no root holds, at all times, something above itself: a chain never
// repeats a slot and has at most n links.  Two orders instantiate this.  Components: the index order, descending
// (the local kernel writes values <= the index; merge and flatten only ever lower a slot).  Basins: the key order
// (height, -index), ascending (key(parent(v)) > key(v); flatten replaces a slot only by an ancestor).  Whatever a
// walker reads in a slot is an ancestor of that slot, so races change the path, never the end.  No index is followed
// before it is checked against n, and nothing but a slot that holds its own index ends the walk well: a slot that
// cannot occur, or n links without a root, sets *overrun and gives -1.
__device__ __forceinline__ int find_root(const int32_t* slots, int at, int n, int* overrun) {
    for (int it = 0; it < n; ++it) {
        if ((unsigned)at >= (unsigned)n) break;
        const int up = load_slot(slots + at);
        if (up == at) return at;
        at = up;
    }
    *overrun = 1;
    return -1;
}

// The accumulator at the head of the workspace: an entry clears it first and the finish kernel turns it into status.
// A workgroup adds at most one non-zero count and touches the flag only if it overran.  Adds to one address retire at
// about 90 per microsecond on the MI355X, whatever else the kernel does.  The saddle kernel and the basins' flatten add
// as they always did; the labelling entry with 1.2 million roots in 132 k flatten workgroups (700 x 440 x 440) ran 2
// to 10 % behind its parent that way.  So a flatten may be given count words, one per workgroup, behind
// the accumulator: they take the counts with plain stores and the finish kernel sums them.
struct ForestStatus {
    unsigned long long count;                             // roots, or records needed
    int32_t flag;                                         // a loop hit its cap
    int32_t pad;
};
static_assert(sizeof(ForestStatus) == 16, "the head of every entry's workspace");

__device__ __forceinline__ void flag_overrun(ForestStatus* acc) { atomicOr(&acc->flag, 1); }

// slots[v] = find(v), in place, PER voxels per thread.  Slot v is written by its own thread alone, only after a walk
// that ended on a root, and only with that root: a slot that holds its own index is a root at all times and is never
// written.  The workgroup's count of roots goes to block_counts[blockIdx.x], or with block_counts == NULL to the
// accumulator.
template <int PER>
__global__ __launch_bounds__(FOREST_THREADS) void forest_flatten_kernel(int n, int32_t* slots,
                                                                        ForestStatus* __restrict__ acc,
                                                                        int32_t* __restrict__ block_counts) {
    __shared__ int wave_count[FOREST_THREADS / 64];
    int overrun = 0, mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t v = ((int64_t)blockIdx.x * PER + j) * FOREST_THREADS + threadIdx.x;
        if (v >= n) continue;
        const int p = slots[v];                           // only this thread writes slot v in this launch
        if (p < 0) continue;
        if (p == (int)v) {
            mine += 1;
            continue;
        }
        const int r = find_root(slots, p, n, &overrun);
        if (r >= 0 && r != p) store_slot(slots + v, r);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
    overrun = __syncthreads_or(overrun);
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < FOREST_THREADS / 64; ++w) total += wave_count[w];
        if (block_counts) block_counts[blockIdx.x] = total;
        else if (total) atomicAdd(&acc->count, (unsigned long long)total);
        if (overrun) flag_overrun(acc);
    }
}

// One workgroup: status = {flag, the accumulator's count plus the n_counts words at block_counts}, saturating.
__global__ __launch_bounds__(FOREST_THREADS) void forest_finish_kernel(const ForestStatus* __restrict__ acc,
                                                                       const int32_t* __restrict__ block_counts,
                                                                       int64_t n_counts,
                                                                       int32_t* __restrict__ status) {
    __shared__ unsigned long long wave_count[FOREST_THREADS / 64];
    unsigned long long total = 0;
    for (int64_t i = threadIdx.x; i < n_counts; i += FOREST_THREADS) total += (unsigned long long)block_counts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = acc->count;
        for (int w = 0; w < FOREST_THREADS / 64; ++w) sum += wave_count[w];
        status[0] = acc->flag ? 1 : 0;
        status[1] = sum > (unsigned long long)INT_MAX ? INT_MAX : (int32_t)sum;
    }
}

inline hipError_t forest_clear(ForestStatus* acc, hipStream_t st) {
    return hipMemsetAsync(acc, 0, sizeof(ForestStatus), st);
}
inline hipError_t forest_finish(const ForestStatus* acc, const int32_t* block_counts, int64_t n_counts,
                                int32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(forest_finish_kernel, dim3(1), dim3(FOREST_THREADS), 0, st, acc, block_counts, n_counts,
                       status);
    return hipGetLastError();
}
// workgroups of a flatten over n voxels at `per` voxels per thread: the words its block_counts needs
inline int64_t forest_flatten_blocks(int64_t n, int per) {
    return (n + FOREST_THREADS * per - 1) / (FOREST_THREADS * per);
}
// the last two launches of an entry whose forest stands in slots[n]; block_counts: NULL, or a word per workgroup
template <int PER>
hipError_t forest_flatten_and_finish(int n, int32_t* slots, ForestStatus* acc, int32_t* block_counts, int32_t* status,
                                     hipStream_t st) {
    const int64_t blocks = forest_flatten_blocks(n, PER);
    hipLaunchKernelGGL(forest_flatten_kernel<PER>, dim3((unsigned)blocks), dim3(FOREST_THREADS), 0, st, n, slots, acc,
                       block_counts);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : forest_finish(acc, block_counts, block_counts ? blocks : 0, status, st);
}

}  // namespace
