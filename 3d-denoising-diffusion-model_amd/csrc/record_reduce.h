// The two-launch fp64 record reduction of every "figure from a volume" entry: error moments and SSIM
// (metrics.hip), multi-scale SSIM (msssim.hip), trace (trace.hip), roi (roi.hip), the variational bound (ops.hip).
//   1. A streaming kernel has each workgroup reduce its slice into COLS per-thread doubles, and rr_write_record folds
//      them over the workgroup and writes one record of REC doubles to the caller's workspace.
//   2. A fold kernel of one workgroup per output row takes the row's records with rr_fold (record p to thread
//      p mod THREADS, p ascending) and folds the workgroup again: rr_fold_record.
// The order is fixed, and it is the contract: lanes by xor butterfly with offsets 32, 16, .., 1, then the waves in
// ascending order, each column by its own operation.  No atomics, so the same bits on every run, and a row's bits
// depend on that row's records alone: row b of a batch carries the bits of a call on estimate b.
// Records are written with 4-byte stores (halves of the doubles): no wide store whose data registers could be
// rewritten behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// half 0 / 1 of v to the low / high word of *p
__device__ __forceinline__ void store_double(double* p, int lane_half, double v) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    reinterpret_cast<unsigned*>(p)[lane_half] = lane_half ? (unsigned)(bits >> 32) : (unsigned)bits;
}

// A column policy P describes a record: P::REC doubles in the workspace, of which the first P::COLS are reduced (the
// others are written as 0.0), and P::op(k), how column k combines.  RrSum: every column a sum.
enum RrOp { RR_SUM, RR_MIN, RR_MAX };
template <int N, int WIDTH = N>
struct RrSum {
    static constexpr int COLS = N, REC = WIDTH;
    static constexpr RrOp op(int) { return RR_SUM; }
};

// what an empty range leaves in column k
template <class P>
__device__ __forceinline__ constexpr double rr_identity(int k) {
    return P::op(k) == RR_MIN ? (double)INFINITY : P::op(k) == RR_MAX ? -(double)INFINITY : 0.0;
}
template <class P>
__device__ __forceinline__ double rr_combine(int k, double a, double b) {
    return P::op(k) == RR_MIN ? fmin(a, b) : P::op(k) == RR_MAX ? fmax(a, b) : a + b;
}

// The per-wave partials of a workgroup in LDS, as rr_reduce leaves them; total(k) folds column k over the waves in
// ascending order.
template <class P, int THREADS>
struct RrTotals {
    const double (*red)[THREADS / 64];
    __device__ __forceinline__ double operator()(int k) const {
        double tot = red[k][0];
        for (int w = 1; w < THREADS / 64; ++w) tot = rr_combine<P>(k, tot, red[k][w]);
        return tot;
    }
};

// The workgroup tail, for all THREADS threads of the workgroup: folds the P::COLS per-thread values over each wave
// and leaves the waves' partials where every thread can take a column's total (after a barrier).  One use per kernel.
template <class P, int THREADS>
__device__ __forceinline__ RrTotals<P, THREADS> rr_reduce(double (&v)[P::COLS]) {
    __shared__ double red[P::COLS][THREADS / 64];
#pragma unroll
    for (int k = 0; k < P::COLS; ++k)
        v[k] = P::op(k) == RR_MIN ? wave_min(v[k]) : P::op(k) == RR_MAX ? wave_max(v[k]) : wave_sum(v[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < P::COLS; ++k) red[k][wave] = v[k];
    }
    __syncthreads();
    return {red};
}

// The tail, then lane 2k + h stores half h of column k of the record at rec.
template <class P, int THREADS>
__device__ __forceinline__ void rr_write_record(double (&v)[P::COLS], double* __restrict__ rec) {
    const RrTotals<P, THREADS> total = rr_reduce<P, THREADS>(v);
    if (threadIdx.x < 2 * P::REC) {
        const int k = threadIdx.x >> 1;
        store_double(rec + k, threadIdx.x & 1, k < P::COLS ? total(k) : 0.0);
    }
}

// The fold body: this thread's share of the `count` records at `first`, record p = tid, tid + THREADS, .. ascending,
// combined per column from the identity (all an empty range leaves).
template <class P, int THREADS, class Index>
__device__ __forceinline__ void rr_fold(const double* __restrict__ first, Index count, double (&v)[P::COLS]) {
#pragma unroll
    for (int k = 0; k < P::COLS; ++k) v[k] = rr_identity<P>(k);
    for (Index p = threadIdx.x; p < count; p += THREADS) {
        const double* r = first + (size_t)p * P::REC;
#pragma unroll
        for (int k = 0; k < P::COLS; ++k) v[k] = rr_combine<P>(k, v[k], r[k]);
    }
}
template <class P, int THREADS, class Index>
__device__ __forceinline__ void rr_fold_record(const double* __restrict__ first, Index count,
                                               double* __restrict__ out) {
    double v[P::COLS];
    rr_fold<P, THREADS>(first, count, v);
    rr_write_record<P, THREADS>(v, out);
}

// The streaming plan of error moments and trace: `per` = threads * vector width values per workgroup and pass, whole
// passes per workgroup, at most max_parts workgroups per estimate.
struct RrPlan {
    int parts;
    int64_t chunk;
};
inline RrPlan rr_plan(int64_t voxels, int64_t per, int max_parts) {
    const int64_t passes = (voxels + per - 1) / per;
    const int parts = (int)(passes < max_parts ? passes : max_parts);
    const int64_t chunk = (passes + parts - 1) / parts * per;
    return {(int)((voxels + chunk - 1) / chunk), chunk};
}
// an upper bound of the records B estimates write that never shrinks as the volume grows
inline size_t rr_workspace_bytes(int B, int64_t voxels, int64_t per, int max_parts, int rec) {
    const int64_t passes = (voxels + per - 1) / per;
    return (size_t)B * (size_t)(passes < max_parts ? passes : max_parts) * rec * sizeof(double);
}

}  // namespace
