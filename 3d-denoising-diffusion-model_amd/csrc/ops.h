// Internal launcher prototypes (definitions in ops.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the 16-byte (four-wide) forms of a kernel need this of every pointer they read or write
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// the same for a kernel whose pointers need different (power-of-two) alignments
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: raise it once
// per (kernel instantiation, device), not once per process (a process that drives two GPUs would
// otherwise fail its first > 64 KB launch on the second one).  `done` = one flag word per kernel.
struct DynLdsOnce { unsigned long long mask[4]; };   // 256 devices
static inline hipError_t ddpm3d_allow_dynamic_lds(DynLdsOnce& done, const void* kernel, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    dev &= 255;
    unsigned long long& w = done.mask[dev >> 6];
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(&w, __ATOMIC_ACQUIRE) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) __atomic_fetch_or(&w, bit, __ATOMIC_RELEASE);
    return e;
}

hipError_t ddpm3d_launch_pack(const float* w, int Cout, int Cin, int ks, int prec, void* out, hipStream_t st);
hipError_t ddpm3d_launch_pack_up_phase(const float* w, int Cout, int Cin, void* out, hipStream_t st);
hipError_t ddpm3d_launch_gn_finalize(const double* st0, int C0, int rows0, const double* st1, int C1,
                                     int rows1, int N, int groups, double count, float eps,
                                     const float* gamma, const float* beta, const float* film,
                                     int film_stride, int film_off, float* A, float* B, float* bound,
                                     hipStream_t st);
hipError_t ddpm3d_launch_absmax(const float* x0, const float* x1, int N, size_t per_sample, float* bound,
                                hipStream_t st);
hipError_t ddpm3d_launch_gn_stats(const float* x, int N, int voxels, int C, double* stats, hipStream_t st);
int ddpm3d_gn_stats_rows_impl(int voxels);
hipError_t ddpm3d_launch_timestep_embedding(const float* t, int rows, int dim, const float* freqs,
                                            float* out, hipStream_t st);
hipError_t ddpm3d_launch_linear(const float* in, int rows, int K, const float* w, const float* bias, int O,
                                int silu_in, float* out, int out_stride, hipStream_t st);
hipError_t ddpm3d_launch_transpose(const float* in, int N, int R, int S, float* out, hipStream_t st);
hipError_t ddpm3d_launch_to_ndhwc_pad(const float* in, int N, int C, int voxels, int Cpad, float* out, hipStream_t st);
hipError_t ddpm3d_launch_subsample_hw2(const float* in, int N, int D, int H, int W, int C, float* out,
                                       hipStream_t st);
// the step launchers that read noise take it from `key` (noise.h) when one is given, from the tensor otherwise; with
// a non-NULL xs (the *_step_x0 entries) x0 is xs, not derived from mo's first half
struct ddpm3d_noise_key;
hipError_t ddpm3d_launch_sample_step(bool ddim, const float* mo, const float* xs, const float* x, const float* noise,
                                     const ddpm3d_noise_key* key, const float* coef, const int64_t* t_idx, int N,
                                     int voxels, int flags, float eta, float* sample, float* pred_xstart,
                                     hipStream_t st);
// p_mean_variance and the DDIM reverse (inversion) step; T = rows of coef, t outside [0, T) gives NaN
hipError_t ddpm3d_launch_p_mean_variance(const float* mo, const float* x, const float* coef, const int64_t* t_idx,
                                         int N, int voxels, int T, int flags, float* mean, float* variance,
                                         float* log_variance, float* pred_xstart, hipStream_t st);
hipError_t ddpm3d_launch_ddim_reverse_step(const float* mo, const float* x, const float* coef, const int64_t* t_idx,
                                           int N, int voxels, int T, int flags, float* sample, float* pred_xstart,
                                           hipStream_t st);
// one DPM-Solver++ multistep step; scoef = [T][DDPM3D_NSCOEF] weights, m1 / m2 read at order >= 2 / 3, noise may be
// NULL; t outside [0, T) gives NaN
hipError_t ddpm3d_launch_dpm_solver_step(const float* mo, const float* xs, const float* x, const float* m1,
                                         const float* m2, const float* noise, const ddpm3d_noise_key* key,
                                         const float* coef, const float* scoef, const int64_t* t_idx, int N, int voxels,
                                         int T, int flags, int order, float* sample, float* pred_xstart,
                                         hipStream_t st);
// variational bound (calc_bpd_loop): ws holds ddpm3d_vb_parts(voxels) 32-byte records per sample
int ddpm3d_vb_parts(int voxels);
hipError_t ddpm3d_launch_q_sample(const float* x0, const float* noise, const ddpm3d_noise_key* key, const float* qcoef,
                                  const int64_t* t_idx, int N, int voxels, int T, float* xt, hipStream_t st);
hipError_t ddpm3d_launch_vb_terms(const float* mo, const float* x_start, const float* x_t, const float* noise,
                                  const float* coef, const float* qcoef, const int64_t* t_idx, int N, int voxels,
                                  int T, int flags, double* ws, float* vb, float* xstart_mse, float* mse, int ld,
                                  float* pred_xstart, hipStream_t st);
hipError_t ddpm3d_launch_prior_bpd(const float* x_start, const float* qcoef, int N, int voxels, int T, double* ws,
                                   float* out, hipStream_t st);
hipError_t ddpm3d_launch_attention(const float* qkv, int N, int T, int heads, int ch, int precision,
                                   const float* bound, int bound_count, int bound_stride, float* out,
                                   hipStream_t st);
hipError_t ddpm3d_launch_add_embedding(float* emb, const float* table, const int64_t* idx, int rows, int dim,
                                       int num_classes, hipStream_t st);
hipError_t ddpm3d_launch_pool_act(const float* src, const float* A, const float* B, int act, int fast, int N, int D,
                                  int H, int W, int C, float* out, int src16, int out16, int f16, hipStream_t st);
// probe.hip
double ddpm3d_probe_flops_per_iter(int kind);
hipError_t ddpm3d_launch_mfma_probe(int kind, int iters, int blocks, float* out, unsigned long long* clk,
                                    hipStream_t st);
// uncertainty.hip: one patch origin's K draws into acc[K][H][W][D] / wsum[H][W][D] (the caller has checked that the
// origin lies in the volume), and the per-voxel mean / sample std of K accumulators (wsum may be NULL)
hipError_t ddpm3d_launch_draw_stitch(const float* samples, int K, int res, const double* window, int xs, int ys,
                                     int zs, int H, int W, int D, float* acc, float* wsum, hipStream_t st);
hipError_t ddpm3d_launch_draw_moments(const float* acc, const float* wsum, int K, int64_t voxels, float* mean,
                                      float* std, hipStream_t st);
// quantiles.hip: per-voxel quantiles of K accumulators (wsum may be NULL) and the rank of a target among them.  The
// positions travel by value in the kernel arguments; the caller has checked them (lower in 0..K-1, frac in [0, 1),
// frac == 0 at lower == K-1) and that target / below / equal come together and quant with nq > 0
struct ddpm3d_quantile_pos {
    int lower[8];                               // DDPM3D_MAX_QUANTILES (quantiles.hip asserts it)
    float frac[8];
};
hipError_t ddpm3d_launch_draw_quantiles(const float* acc, const float* wsum, int K, int64_t voxels, int nq,
                                        const ddpm3d_quantile_pos& pos, const float* target, float* quant,
                                        uint8_t* below, uint8_t* equal, hipStream_t st);
// metrics.hip: error moments and 3-D SSIM of B estimates against one target (the caller has checked shapes and the
// workspace; the *_workspace_bytes take valid shapes only)
size_t ddpm3d_em_workspace_bytes(int B, int64_t voxels);
hipError_t ddpm3d_launch_error_moments(const float* est, const float* target, const uint8_t* mask, const float* std,
                                       int B, int64_t voxels, double* ws, double* out, hipStream_t st);
size_t ddpm3d_ss_workspace_bytes(int B, int D, int H, int W);
hipError_t ddpm3d_launch_ssim3d(const float* est, const float* target, const uint8_t* mask, int B, int D, int H, int W,
                                float C1, float C2, double* ws, float* map, double* out, hipStream_t st);
// trace.hip: weighted moments of B estimates against their targets and the previous estimates (the caller has checked
// the pointers, the strides (0 or voxels) and the workspace; the workspace query takes valid shapes only)
size_t ddpm3d_tr_workspace_bytes(int B, int64_t voxels);
hipError_t ddpm3d_launch_trace_moments(const float* est, const float* prev, const float* target, const float* weight,
                                       int B, int64_t voxels, int64_t target_stride, int64_t weight_stride, double* ws,
                                       double* out, hipStream_t st);
// msssim.hip: 2 x 2 x 2 mean pooling of B volumes (and of one mask, by the 4-of-8 rule), and the multi-scale SSIM of B
// estimates against one target: per scale the SSIM parts launch and its fold into out[B][scales][3], then the pools
// into ws (the caller has checked the shapes, that every extent >> (scales - 1) is at least 11, and the workspace)
hipError_t ddpm3d_launch_pool2(const float* vol, const uint8_t* mask, int B, int D, int H, int W, float* out,
                               uint8_t* mask_out, hipStream_t st);
size_t ddpm3d_ms_workspace_bytes(int B, int D, int H, int W, int scales);
hipError_t ddpm3d_launch_msssim3d(const float* est, const float* target, const uint8_t* mask, int B, int D, int H,
                                  int W, int scales, float C1, float C2, void* ws, double* out, hipStream_t st);
// roi.hip: per-region moments over a region index cut into `chunks` chunks in all (the caller has checked the
// descriptor's host side and the workspace)
struct ddpm3d_roi_index;
hipError_t ddpm3d_launch_roi_moments(const float* est, const float* target, int B, int64_t voxels,
                                     const ddpm3d_roi_index& ix, int64_t chunks, double* ws, double* out,
                                     hipStream_t st);
// texture.hip: per-region co-occurrence matrices, histograms and side counters over the same index; zeroes the three
// outputs on `st` first (the caller has checked the descriptor's host side, the shape and the level count)
hipError_t ddpm3d_launch_roi_texture(const float* est, int B, int D, int H, int W, const ddpm3d_roi_index& ix,
                                     int64_t chunks, const int16_t* region_of, const float* lo, const float* inv_w,
                                     int levels, uint64_t* glcm, uint64_t* hist, uint64_t* counts, hipStream_t st);
// spectrum.hip: the windowed 3-D DFT as three MFMA GEMM passes, the per-shell sums over a shell index cut into
// `chunks` chunks, and the driver of both (the caller has checked the shapes, the axis tables, the descriptor's host
// side and the workspaces; the workspace queries take valid shapes only).  only = 0, 1, 2 runs pass W, H or D alone, -1 all.
struct ddpm3d_dft_axis;
size_t ddpm3d_dft_workspace_bytes(int B, int D, int H, int W);
hipError_t ddpm3d_launch_dft3(const float* vol, const float* pivot, int B, int D, int H, int W,
                              const ddpm3d_dft_axis* axes, void* ws, float* re, float* im, int only, hipStream_t st);
size_t ddpm3d_sp_workspace_bytes(int B, int64_t chunks);
hipError_t ddpm3d_launch_shell_sums(const float* xre, const float* xim, const float* yre, const float* yim, int B,
                                    int D, int H, int W, const ddpm3d_roi_index& ix, int64_t chunks, double* ws,
                                    double* out, hipStream_t st);
size_t ddpm3d_spectrum_workspace_bytes(int B, int D, int H, int W, int64_t chunks, int with_target);
hipError_t ddpm3d_launch_shell_spectrum(const float* est, const float* est_pivot, const float* target,
                                        const float* target_pivot, int B, int D, int H, int W,
                                        const ddpm3d_dft_axis* axes, const ddpm3d_roi_index& ix, int64_t chunks,
                                        void* ws, double* out, hipStream_t st);
// ccl.hip: connected components of vol > threshold (the caller has checked the shape, the connectivity and the
// workspace: voxel_forest.h's 16-byte status accumulator and a count word per flatten workgroup; the workspace query
// takes valid shapes only)
size_t ddpm3d_ccl_workspace_bytes(int D, int H, int W);
hipError_t ddpm3d_launch_label_components(const float* vol, const uint8_t* keep, float threshold, int connectivity,
                                          int D, int H, int W, int32_t* roots, void* ws, int32_t* status,
                                          hipStream_t st);
// peak.hip: the sphere-mean map of B volumes (the caller has checked the shape, the radii and the table, whose
// entries lie in -1..DDPM3D_PEAK_MAX_RADIUS)
hipError_t ddpm3d_launch_sphere_mean(const float* vol, const uint8_t* keep, int B, int D, int H, int W, int r0, int r1,
                                     const int32_t* half_w, float* out, hipStream_t st);
// smooth.hip: the separable Gaussian of one volume, passes along W, H, D (the caller has checked the shape, the radii
// (D, H, W order, 0..DDPM3D_SMOOTH_MAX_RADIUS), the three host tap tables and the workspace of one volume)
hipError_t ddpm3d_launch_gauss_smooth(const float* vol, int D, int H, int W, const int* radii, const float* const* taps,
                                      float* out, float* ws, hipStream_t st);
// guide.hip: x0 = clip(x0_raw + weight * G(y - x0_raw)) of N samples, G as above and batched (the caller has checked
// the shape, the radii, the taps, the weight and the workspace of N volumes); t outside [0, T) gives NaN
hipError_t ddpm3d_launch_xstart_pull(const float* mo, const float* x, const float* y, const float* coef,
                                     const int64_t* t_idx, int N, int D, int H, int W, int T, int flags, float weight,
                                     const int* radii, const float* const* taps, float* out, float* ws,
                                     hipStream_t st);
// nlm.hip: non-local means of one volume (the caller has checked the shape and the radii); the weight of a candidate
// is exp(-max(fma(sum of squared patch differences, k1, -k2), 0)), k1 = 1 / (n_p h^2), k2 = 2 sigma^2 / h^2
hipError_t ddpm3d_launch_nlm(const float* vol, int D, int H, int W, const int* search, const int* patch, float k1,
                             float k2, float* out, hipStream_t st);
// project.hip: the maximum (mode DDPM3D_PROJECT_MAX) or the line integral (DDPM3D_PROJECT_SUM) along the table's rays
// through every slice of B volumes, out [B][angles][D][bins] (the caller has checked the shape, the table and the mode)
struct ddpm3d_project_table;
hipError_t ddpm3d_launch_project(const float* vol, int B, int D, int H, int W, const ddpm3d_project_table& table,
                                 int mode, float* out, hipStream_t st);
// edt.hip: the squared distance in mm^2 from every foreground voxel ((mask != 0) != invert) of K volumes to the nearest
// background voxel of its volume, s[] the fp32 spacings along D, H, W; three launches, the last two in place on out
// (the caller has checked the shape, the spacings and invert)
hipError_t ddpm3d_launch_distance_sq(const uint8_t* mask, int K, int D, int H, int W, int invert, const float s[3],
                                     float* out, hipStream_t st);
// watershed.hip: peaks[v] = the peak that steepest ascent under key (height, -index) reaches from v within v's label,
// and the records (a < b, min of the two heights) of neighbouring voxels in different basins, reduced per workgroup;
// at most `cap` records are written, all are counted (the caller has checked the shape, the connectivity, the capacity
// and the workspace of ddpm3d_watershed_workspace_bytes() bytes, the same status accumulator, which both entries use)
size_t ddpm3d_watershed_workspace_bytes();
hipError_t ddpm3d_launch_basins(const float* height, const int32_t* labels, int connectivity, int D, int H, int W,
                                int32_t* peaks, void* ws, int32_t* status, hipStream_t st);
hipError_t ddpm3d_launch_basin_saddles(const float* height, const int32_t* labels, const int32_t* peaks,
                                       int connectivity, int D, int H, int W, int cap, int32_t* pairs, float* saddle,
                                       void* ws, int32_t* status, hipStream_t st);
// regrid.hip: B volumes of one shape onto another grid, passes along W, H, D with the tables of axes[] (D, H, W order)
// in device memory (the caller has checked the shapes, the taps, the ratios and the workspace); stage[] gets the voxels
// per volume after the W, the H and the D pass, of which the first two, times B, are the workspace's two buffers
struct ddpm3d_regrid_axis;
void ddpm3d_regrid_stages(int D, int H, int W, int Do, int Ho, int Wo, int64_t stage[3]);
hipError_t ddpm3d_launch_regrid(const float* vol, int B, int D, int H, int W, const ddpm3d_regrid_axis* axes,
                                float* out, float* ws, hipStream_t st);
// tiling.hip: B canvases (Dc, H, W) -> rows [first_patch * B, (first_patch + n_patches) * B) of the (patch, draw)-major
// patch tensor, and all patches -> B canvases with the normalised Hann blend (the caller has checked the geometry).
// One gather and one blend kernel, instantiated for starts in the kernel arguments (joint: at most
// DDPM3D_JOINT_MAX_STARTS per axis) ...
struct ddpm3d_joint_starts;
hipError_t ddpm3d_launch_joint_gather(const float* canvas, int B, int Dc, int H, int W, int res,
                                      const ddpm3d_joint_starts& s, int first_patch, int n_patches, float* out,
                                      hipStream_t st);
hipError_t ddpm3d_launch_joint_blend(const float* patches, int B, int Dc, int H, int W, int res,
                                     const ddpm3d_joint_starts& s, const double* tables, float* out, hipStream_t st);
// ... and for starts and a per-coordinate cover lookup in device memory (tiles: any number per axis)
struct ddpm3d_tiling;
hipError_t ddpm3d_launch_tiles_gather(const float* canvas, int B, int Dc, int H, int W, int res,
                                      const ddpm3d_tiling& t, int first_patch, int n_patches, float* out,
                                      hipStream_t st);
hipError_t ddpm3d_launch_tiles_blend(const float* patches, int B, int Dc, int H, int W, int res,
                                     const ddpm3d_tiling& t, float* out, hipStream_t st);
