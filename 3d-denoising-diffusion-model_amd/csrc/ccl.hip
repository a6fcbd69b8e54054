// Connected-component labelling of a thresholded volume (definitions in include/ddpm3d.h):
// roots[v] = flat index of the lowest-index voxel of v's component, -1 for background.  A clear of the 16-byte status
// accumulator and four launches on one stream; the walk, flatten and finish are voxel_forest.h's:
//   local    one workgroup per brick of DDPM3D_CCL_TILE_D x _H x _W voxels labels the brick in LDS and writes, per
//            voxel, the global index of its brick-local root: a forest of depth 1 with roots[v] <= v
//   merge    every foreground voxel on a brick's low face unites its tree with those of its foreground neighbours in
//            other bricks: atomicMin on root slots only
//   flatten  roots[v] = find(v); every workgroup stores its count of roots in its word behind the accumulator
//   finish   one workgroup sums the count words and writes the sum and the accumulator's cap flag into status[2]
// No workgroup waits for another.  Every loop walks a strictly decreasing chain of indices, so it ends; each also
// counts its iterations against a cap that a correct run cannot reach and that sets the accumulator's flag.
// The answer is a property of the input alone (the minimum of each component), whatever order the atomics land in.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "ddpm3d.h"
#include "ops.h"
#include "voxel_forest.h"

namespace {

constexpr int TD = DDPM3D_CCL_TILE_D, TH = DDPM3D_CCL_TILE_H, TW = DDPM3D_CCL_TILE_W;
constexpr int CCL_THREADS = 256;
constexpr int BRICK = TD * TH * TW;
constexpr int PER = BRICK / CCL_THREADS;                  // voxels per thread of the local kernel
constexpr int PH = TH + 2, PW = TW + 2;                   // the brick in LDS carries a one-voxel background halo
constexpr int PADDED = (TD + 2) * PH * PW;
constexpr int NONE = INT_MAX;                             // background in LDS: never the minimum
constexpr int FLAT_PER = 4;                               // voxels per thread of the flatten kernel
static_assert(CCL_THREADS == FOREST_THREADS, "one launch width");
static_assert(TW == 64 && BRICK % CCL_THREADS == 0, "a wave takes one full line of the brick");
static_assert(PADDED * 4 <= 32 * 1024, "the brick's labels stay well under the 64 KB a workgroup may take");

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
                                                                Extents g, int bh, int bw,
                                                                int32_t* __restrict__ roots,
                                                                ForestStatus* __restrict__ acc) {
    __shared__ int L[PADDED];
    const int tid = threadIdx.x;
    const int brick = blockIdx.x;
    const int bx = brick % bw, by = (brick / bw) % bh, bz = brick / (bw * bh);
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
    if (tid == 0 && overrun) flag_overrun(acc);
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
        if (a == b || a < 0 || b < 0) return;             // one tree, or a walk that failed: nothing to link
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
__global__ __launch_bounds__(CCL_THREADS) void ccl_merge_kernel(Extents g, int n, int32_t* roots,
                                                                ForestStatus* __restrict__ acc) {
    const int64_t v64 = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
    int overrun = 0;
    if (v64 < n) {
        const int v = (int)v64;
        const Voxel at = voxel_of(g, v);
        const int z = at.z, y = at.y, x = at.x;
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
    if (overrun) flag_overrun(acc);
}

template <int ORDER>
hipError_t launch(const float* vol, const uint8_t* keep, float threshold, Extents g, int32_t* roots, ForestStatus* acc,
                  int32_t* status, hipStream_t st) {
    const int n = (int)((int64_t)g.D * g.H * g.W);
    // bricks along each axis; extents reach 2^31 - 1: no "+ tile - 1"
    const int bd = (g.D - 1) / TD + 1, bh = (g.H - 1) / TH + 1, bw = (g.W - 1) / TW + 1;
    hipError_t e = forest_clear(acc, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ccl_local_kernel<ORDER>, dim3((unsigned)((int64_t)bd * bh * bw)), dim3(CCL_THREADS), 0, st, vol,
                       keep, threshold, g, bh, bw, roots, acc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ccl_merge_kernel<ORDER>, dim3((unsigned)(((int64_t)n + CCL_THREADS - 1) / CCL_THREADS)),
                       dim3(CCL_THREADS), 0, st, g, n, roots, acc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return forest_flatten_and_finish<FLAT_PER>(n, roots, acc, (int32_t*)(acc + 1), status, st);
}

}  // namespace

// the accumulator, then a count word per flatten workgroup
size_t ddpm3d_ccl_workspace_bytes(int D, int H, int W) {
    const size_t words = (size_t)forest_flatten_blocks((int64_t)D * H * W, FLAT_PER);
    return sizeof(ForestStatus) + ((words * sizeof(int32_t) + 15) & ~(size_t)15);
}

hipError_t ddpm3d_launch_label_components(const float* vol, const uint8_t* keep, float threshold, int connectivity,
                                          int D, int H, int W, int32_t* roots, void* ws, int32_t* status,
                                          hipStream_t st) {
    return with_order(connectivity, [&](auto order) {
        return launch<decltype(order)::value>(vol, keep, threshold, {D, H, W}, roots, (ForestStatus*)ws, status, st);
    });
}
