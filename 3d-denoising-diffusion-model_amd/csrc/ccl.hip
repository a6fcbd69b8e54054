// Connected-component labelling of a thresholded volume (definitions in include/ddpm3d.h):
// roots[v] = flat index of the lowest-index voxel of v's component, -1 for background.  Four launches on one stream:
//   local    one workgroup per brick of DDPM3D_CCL_TILE_D x _H x _W voxels labels the brick in LDS and writes, per
//            voxel, the global index of its brick-local root: a forest of depth 1 with roots[v] <= v
//   merge    every foreground voxel on a brick's low face unites its tree with those of its foreground neighbours in
//            other bricks: atomicMin on root slots only
//   flatten  roots[v] = find(v); every workgroup writes its count of roots to the workspace
//   fold     one workgroup sums the counts and ors the cap flags into status[2]
// No workgroup waits for another.  Every loop walks a strictly decreasing chain of indices, so it ends; each also
// counts its iterations against a cap that a correct run cannot reach and leaves with the workgroup's flag set.
// The answer is a property of the input alone (the minimum of each component), whatever order the atomics land in.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"

namespace {

constexpr int TD = DDPM3D_CCL_TILE_D, TH = DDPM3D_CCL_TILE_H, TW = DDPM3D_CCL_TILE_W;
constexpr int CCL_THREADS = 256;
constexpr int BRICK = TD * TH * TW;
constexpr int PER = BRICK / CCL_THREADS;                  // voxels per thread of the local kernel
constexpr int PH = TH + 2, PW = TW + 2;                   // the brick in LDS carries a one-voxel background halo
constexpr int PADDED = (TD + 2) * PH * PW;
constexpr int NONE = INT_MAX;                             // background in LDS: never the minimum
constexpr int FLAT_PER = 4;                               // voxels per thread of the flatten kernel
static_assert(TW == 64 && BRICK % CCL_THREADS == 0, "a wave takes one full line of the brick");
static_assert(PADDED * 4 <= 32 * 1024, "the brick's labels stay well under the 64 KB a workgroup may take");

struct Dims {
    int D, H, W;
    int bh, bw;            // bricks along H and W
};

// The neighbours of a connectivity, as offsets in the padded brick: those with at most `order` non-zero components.
template <int ORDER, typename F>
__device__ __forceinline__ void for_neighbours(F&& f) {
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int nz = (dz != 0) + (dy != 0) + (dx != 0);
                if (nz >= 1 && nz <= ORDER) f(dz, dy, dx);
            }
}

__device__ __forceinline__ int load_slot(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Walks parent slots from v to a slot that holds its own index.  Every slot u holds a value <= u at all times (the
// local kernel writes such values; merge and flatten only ever lower a slot), so the chain strictly decreases and has
// at most v + 1 links: the loop ends.  `cap` (the voxel count) is therefore out of reach; hitting it sets *overrun.
__device__ __forceinline__ int find_root(const int32_t* roots, int v, int cap, int* overrun) {
    int at = v;
    for (int it = 0; it < cap; ++it) {
        const int up = load_slot(roots + at);
        if (up >= at || up < 0) return at;      // its own index: a root (anything else there is not a chain: stop)
        at = up;
    }
    *overrun = 1;
    return at;
}

// ---------------------------------------------------------------------------------------------------- local
// L[p] for a padded index p: p itself for a foreground voxel at first, NONE for background and the halo.  Padded
// indices order the brick's voxels as flat indices order them, so "lowest padded index" is "lowest flat index".
// One round: (A) every foreground voxel takes the minimum of its own and its in-brick neighbours' labels, then (B)
// replaces its label by the root of that label's chain.  Reads and writes of a phase are split by a barrier, so
// each phase works on a snapshot: no data race, and the same rounds on every run.
// Invariant: L[p] <= p and L[p] lies in p's component.  A and B only lower labels.  When A changes nothing, every
// voxel's label is <= each neighbour's, hence equal along every edge, hence constant on the component; the
// component's minimum m has L[m] <= m in the component, so L[m] = m and the constant is m.
// Bound: without B, after k rounds a voxel holds at most the minimum within k steps; B only lowers further and A is
// monotone, so at most BRICK - 1 rounds change anything and round BRICK sees no change.  The cap is BRICK + 1.
template <int ORDER>
__global__ __launch_bounds__(CCL_THREADS) void ccl_local_kernel(const float* __restrict__ vol,
                                                                const uint8_t* __restrict__ keep, float threshold,
                                                                Dims g, int32_t* __restrict__ roots,
                                                                int32_t* __restrict__ flags) {
    __shared__ int L[PADDED];
    const int tid = threadIdx.x;
    const int brick = blockIdx.x;
    const int bx = brick % g.bw, by = (brick / g.bw) % g.bh, bz = brick / (g.bw * g.bh);
    const int z0 = bz * TD, y0 = by * TH, x0 = bx * TW;

    for (int p = tid; p < PADDED; p += CCL_THREADS) L[p] = NONE;
    __syncthreads();

    const int x = tid & (TW - 1);
    unsigned fg = 0;                                      // bit j: my j-th voxel is foreground
    int64_t at[PER];                                      // its flat index, -1 outside the volume
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int row = (tid >> 6) + j * (CCL_THREADS / TW);
        const int z = row / TH, y = row % TH;
        const bool inside = z0 + z < g.D && y0 + y < g.H && x0 + x < g.W;
        at[j] = inside ? ((int64_t)(z0 + z) * g.H + (y0 + y)) * g.W + (x0 + x) : -1;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (at[j] < 0) continue;
        bool on = vol[at[j]] > threshold;                 // false for NaN
        if (keep) on = on && keep[at[j]] != 0;
        if (on) fg |= 1u << j;
    }
    auto padded = [&](int j) {
        const int row = (tid >> 6) + j * (CCL_THREADS / TW);
        return ((row / TH + 1) * PH + (row % TH + 1)) * PW + x + 1;
    };
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (fg >> j & 1) L[padded(j)] = padded(j);
    __syncthreads();

    int overrun = 1;
    for (int round = 0; round <= BRICK; ++round) {
        int next[PER];
        int changed = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {                   // A, reads
            if (!(fg >> j & 1)) continue;
            const int p = padded(j);
            const int mine = L[p];
            int m = mine;
            for_neighbours<ORDER>([&](int dz, int dy, int dx) { m = min(m, L[p + (dz * PH + dy) * PW + dx]); });
            next[j] = m;
            changed |= m < mine;
        }
        changed = __syncthreads_or(changed);
        if (!changed) {
            overrun = 0;
            break;
        }
#pragma unroll
        for (int j = 0; j < PER; ++j)                     // A, writes
            if (fg >> j & 1) L[padded(j)] = next[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {                   // B, reads: L[l] <= l, so the chain ends within PADDED links
            if (!(fg >> j & 1)) continue;
            int l = next[j];
            for (int it = 0; it < PADDED; ++it) {
                const int up = L[l];
                if (up >= l) break;
                l = up;
            }
            next[j] = l;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j)                     // B, writes
            if (fg >> j & 1) L[padded(j)] = next[j];
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (at[j] < 0) continue;
        int32_t out = -1;
        if (fg >> j & 1) {
            const int l = L[padded(j)];
            const int lz = l / (PH * PW) - 1, ly = l / PW % PH - 1, lx = l % PW - 1;
            out = (int32_t)(((int64_t)(z0 + lz) * g.H + (y0 + ly)) * g.W + (x0 + lx));
        }
        roots[at[j]] = out;
    }
    if (tid == 0) flags[brick] = overrun;
}

// ---------------------------------------------------------------------------------------------------- merge
// Unites the trees of a and b.  Per pass: find both roots; equal -> done; else atomicMin the larger root's slot with
// the smaller.  If the slot still held its own index the link is made.  If not, another thread lowered it first; the
// value it now holds is below the larger root, and the pass repeats from there.  Each repeat strictly lowers
// (larger root, smaller root) in lexicographic order, so there are at most 2 n passes; the cap is out of reach.
// Stale reads are harmless: a slot's older value is still an ancestor in the same tree, and only the atomicMin, which
// acts on the slot's true value, ever links.
__device__ __forceinline__ void unite(int32_t* roots, int a, int b, int cap, int* overrun) {
    for (int it = 0; it < cap; ++it) {
        a = find_root(roots, a, cap, overrun);
        b = find_root(roots, b, cap, overrun);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(roots + a, b);
        if (old == a) return;
        a = old;                                          // a was no root any more: go on from its parent, old < a
    }
    *overrun = 1;
}

// One thread per voxel; it works only if its voxel is foreground and lies on the low face of its brick along some
// axis (not on the volume's own low face).  Two neighbours in different bricks differ in their brick coordinate
// along some axis, and the one with the higher coordinate is on its brick's low face there: every pair across a
// brick border is seen from at least one side.  In-brick pairs are the local kernel's.
template <int ORDER>
__global__ __launch_bounds__(CCL_THREADS) void ccl_merge_kernel(Dims g, int n, int32_t* roots,
                                                                int32_t* __restrict__ flags) {
    const int64_t v64 = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
    int overrun = 0;
    if (v64 < n) {
        const int v = (int)v64;
        const int x = v % g.W, y = v / g.W % g.H, z = v / g.W / g.H;
        const bool face = (z % TD == 0 && z > 0) || (y % TH == 0 && y > 0) || (x % TW == 0 && x > 0);
        if (face && load_slot(roots + v) >= 0) {
            for_neighbours<ORDER>([&](int dz, int dy, int dx) {
                const int nz = z + dz, ny = y + dy, nx = x + dx;
                if (nz < 0 || nz >= g.D || ny < 0 || ny >= g.H || nx < 0 || nx >= g.W) return;
                if (nz / TD == z / TD && ny / TH == y / TH && nx / TW == x / TW) return;
                const int u = (int)(((int64_t)nz * g.H + ny) * g.W + nx);
                if (load_slot(roots + u) >= 0) unite(roots, v, u, n, &overrun);
            });
        }
    }
    overrun = __syncthreads_or(overrun);
    if (threadIdx.x == 0) flags[blockIdx.x] = overrun;
}

// ---------------------------------------------------------------------------------------------------- flatten
// roots[v] = find(v), in place.  A slot that holds its own index is a root and is never written; any other slot is
// only ever replaced by its tree's root, which is below it: find_root's invariant holds while other threads write,
// and a slot equal to its index is a true root at all times, so every walk ends at the one right answer.
__global__ __launch_bounds__(CCL_THREADS) void ccl_flatten_kernel(int n, int32_t* roots, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ flags) {
    __shared__ int wave_count[CCL_THREADS / 64];
    int overrun = 0, mine = 0;
#pragma unroll
    for (int j = 0; j < FLAT_PER; ++j) {
        const int64_t v = ((int64_t)blockIdx.x * FLAT_PER + j) * CCL_THREADS + threadIdx.x;
        if (v >= n) continue;
        const int p = roots[v];                           // only this thread writes slot v in this launch
        if (p < 0) continue;
        if (p == (int)v) {
            mine += 1;
            continue;
        }
        const int r = find_root(roots, p, n, &overrun);
        if (r != p) __hip_atomic_store(roots + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
    overrun = __syncthreads_or(overrun);
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < CCL_THREADS / 64; ++w) total += wave_count[w];
        counts[blockIdx.x] = total;
        flags[blockIdx.x] = overrun;
    }
}

// One workgroup: status[0] = any of the n_flags words set, status[1] = sum of the n_counts words (at most n < 2^31).
__global__ __launch_bounds__(CCL_THREADS) void ccl_fold_kernel(const int32_t* __restrict__ counts, int64_t n_counts,
                                                               const int32_t* __restrict__ flags, int64_t n_flags,
                                                               int32_t* __restrict__ status) {
    __shared__ int wave_count[CCL_THREADS / 64];
    int total = 0, any = 0;
    for (int64_t i = threadIdx.x; i < n_counts; i += CCL_THREADS) total += counts[i];
    for (int64_t i = threadIdx.x; i < n_flags; i += CCL_THREADS) any |= flags[i] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = total;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < CCL_THREADS / 64; ++w) sum += wave_count[w];
        status[0] = any ? 1 : 0;
        status[1] = sum;
    }
}

struct Plan {
    int64_t bricks, merge_blocks, flat_blocks;
    Dims g;
};

Plan plan_of(int D, int H, int W) {
    Plan p;
    const int64_t n = (int64_t)D * H * W;
    p.g = {D, H, W, (H - 1) / TH + 1, (W - 1) / TW + 1};       // extents reach 2^31 - 1: no "+ tile - 1"
    p.bricks = (int64_t)((D - 1) / TD + 1) * p.g.bh * p.g.bw;
    p.merge_blocks = (n + CCL_THREADS - 1) / CCL_THREADS;
    p.flat_blocks = (n + CCL_THREADS * FLAT_PER - 1) / (CCL_THREADS * FLAT_PER);
    return p;
}

template <int ORDER>
hipError_t launch(const float* vol, const uint8_t* keep, float threshold, const Plan& p, int n, int32_t* roots,
                  int32_t* ws, int32_t* status, hipStream_t st) {
    int32_t* counts = ws;                                 // [flat_blocks], then the flag words of the three launches
    int32_t* flags = counts + p.flat_blocks;
    hipLaunchKernelGGL(ccl_local_kernel<ORDER>, dim3((unsigned)p.bricks), dim3(CCL_THREADS), 0, st, vol, keep,
                       threshold, p.g, roots, flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ccl_merge_kernel<ORDER>, dim3((unsigned)p.merge_blocks), dim3(CCL_THREADS), 0, st, p.g, n,
                       roots, flags + p.bricks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)p.flat_blocks), dim3(CCL_THREADS), 0, st, n, roots, counts,
                       flags + p.bricks + p.merge_blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ccl_fold_kernel, dim3(1), dim3(CCL_THREADS), 0, st, counts, p.flat_blocks, flags,
                       p.bricks + p.merge_blocks + p.flat_blocks, status);
    return hipGetLastError();
}

}  // namespace

size_t ddpm3d_ccl_workspace_bytes(int D, int H, int W) {
    const Plan p = plan_of(D, H, W);
    const size_t words = (size_t)(p.bricks + p.merge_blocks + 2 * p.flat_blocks);
    return (words * sizeof(int32_t) + 15) & ~(size_t)15;
}

hipError_t ddpm3d_launch_label_components(const float* vol, const uint8_t* keep, float threshold, int connectivity,
                                          int D, int H, int W, int32_t* roots, void* ws, int32_t* status,
                                          hipStream_t st) {
    const Plan p = plan_of(D, H, W);
    const int n = (int)((int64_t)D * H * W);
    if (connectivity == 6) return launch<1>(vol, keep, threshold, p, n, roots, (int32_t*)ws, status, st);
    if (connectivity == 18) return launch<2>(vol, keep, threshold, p, n, roots, (int32_t*)ws, status, st);
    return launch<3>(vol, keep, threshold, p, n, roots, (int32_t*)ws, status, st);
}
