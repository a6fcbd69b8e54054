// C ABI (include/ddpm3d.h): argument validation + launcher calls.  Nothing
// here allocates or synchronises; every entry point only enqueues on `stream`.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "conv3d_select.h"
#include "ddpm3d.h"
#include "ops.h"
#include "noise.h"

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int launched(hipError_t e, const char* what) {
    if (e == hipSuccess) return DDPM3D_OK;
    return fail(DDPM3D_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
}

extern "C" {

int ddpm3d_abi_version(void) { return DDPM3D_ABI_VERSION; }
const char* ddpm3d_last_error(void) { return g_err; }

static bool prec_ok(int p) { return p >= DDPM3D_PREC_F32 && p <= DDPM3D_PREC_BF16_WZ; }
// modes whose activation scale comes from in_bound (the bf16 modes need none: fp32's exponent range)
static bool prec_scaled(int p) { return p != DDPM3D_PREC_F32 && p != DDPM3D_PREC_BF16 && p != DDPM3D_PREC_BF16_WZ; }

// the Winograd-D form exists for 3x3x3 layers whose couts fill whole 128-wide workgroups
static bool wz_layer_ok(int Cout, int Cin, int ksize) {
    return ksize == 3 && Cout % 128 == 0 && Cin % DDPM3D_CONV_CK == 0;
}

size_t ddpm3d_packed_weight_bytes(int Cout, int Cin, int ksize, int precision) {
    if (Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3) || !prec_ok(precision)) return 0;
    if (ddpm3d_prec_wz(precision) && !wz_layer_ok(Cout, Cin, ksize)) return 0;
    return ddpm3d_packed_image(Cout, Cin, ksize, precision).bytes();
}

int ddpm3d_pack_conv_weight(const float* w, int Cout, int Cin, int ksize, int precision, void* out,
                            void* stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3) || !prec_ok(precision))
        return fail(DDPM3D_EINVAL, "pack_conv_weight: bad arguments (Cout=%d Cin=%d k=%d precision=%d)", Cout,
                    Cin, ksize, precision);
    if (!aligned16(out)) return fail(DDPM3D_EINVAL, "pack_conv_weight: w_packed must be 16-byte aligned");
    if (ddpm3d_prec_wz(precision) && !wz_layer_ok(Cout, Cin, ksize))
        return fail(DDPM3D_ENOSUP, "pack_conv_weight: the Winograd-D form needs ksize 3, Cout %% 128 == 0, "
                                   "Cin %% 16 == 0 (got Cout=%d Cin=%d k=%d)", Cout, Cin, ksize);
    return launched(ddpm3d_launch_pack(w, Cout, Cin, ksize, precision, out, (hipStream_t)stream),
                    "pack_conv_weight");
}

size_t ddpm3d_packed_up_phase_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0 || !wz_layer_ok(Cout, Cin, 3)) return 0;
    return ddpm3d_up_phase_bytes(Cout, Cin);
}

int ddpm3d_pack_up_phase_weight(const float* w, int Cout, int Cin, void* out, void* stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0)
        return fail(DDPM3D_EINVAL, "pack_up_phase_weight: bad arguments (Cout=%d Cin=%d)", Cout, Cin);
    if (!aligned16(out)) return fail(DDPM3D_EINVAL, "pack_up_phase_weight: w_packed must be 16-byte aligned");
    if (!wz_layer_ok(Cout, Cin, 3))
        return fail(DDPM3D_ENOSUP, "pack_up_phase_weight: needs Cout %% 128 == 0, Cin %% 16 == 0 (got Cout=%d Cin=%d)",
                    Cout, Cin);
    return launched(ddpm3d_launch_pack_up_phase(w, Cout, Cin, out, (hipStream_t)stream), "pack_up_phase_weight");
}

int ddpm3d_conv_stats_rows(int N, int D, int H, int W, int Cin, int Cout, int ksize, int precision) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !prec_ok(precision)) return 0;
    return ddpm3d_conv_cfg(N, D, H, W, Cin, Cout, ksize, precision).stats_rows;
}

size_t ddpm3d_conv_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int ksize, int precision) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !prec_ok(precision)) return 0;
    return ddpm3d_conv_cfg(N, D, H, W, Cin, Cout, ksize, precision).workspace_bytes;
}

// Validation shared by ddpm3d_conv3d and the queries: the checks in their order, the launch record, and -- from
// ddpm3d_conv_select, which alone decides it -- the kernel instance that takes the call.  skip_cx: conv3d_select.h.
static int conv_prepare(const ddpm3d_conv_desc* d, ConvK& k, ConvCfg& c, ConvSel& s, bool for_launch, int skip_cx = 0) {
    if (!d) return fail(DDPM3D_EINVAL, "conv3d: null descriptor");
    if (d->N <= 0 || d->D <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0 || d->Cin <= 0)
        return fail(DDPM3D_EINVAL, "conv3d: non-positive shape N=%d D=%d H=%d W=%d Cin=%d Cout=%d", d->N, d->D,
                    d->H, d->W, d->Cin, d->Cout);
    if (d->ksize != 1 && d->ksize != 3) return fail(DDPM3D_EINVAL, "conv3d: ksize %d (1 or 3)", d->ksize);
    if (!prec_ok(d->precision)) return fail(DDPM3D_ENOSUP, "conv3d: precision mode %d not implemented", d->precision);
    if (d->C0 + d->C1 != d->Cin) return fail(DDPM3D_EINVAL, "conv3d: C0+C1 != Cin");
    // (a family query may come before the caller has attached its per-call buffers)
    if (for_launch && (!d->src0 || !d->w_packed || !d->bias || !d->out)) return fail(DDPM3D_EINVAL, "conv3d: null buffer");
    if (d->in_mode == DDPM3D_IN_PLANAR2) {
        if (d->Cin != 2 || d->C0 != 1 || d->C1 != 1 || (for_launch && !d->src1) || d->aff_a)
            return fail(DDPM3D_EINVAL, "conv3d: planar2 input needs C0=C1=1, two planes, no affine");
    } else {
        if (d->in_mode < 0 || d->in_mode > DDPM3D_IN_STRIDE2) return fail(DDPM3D_EINVAL, "conv3d: in_mode %d", d->in_mode);
        if (d->in_mode == DDPM3D_IN_STRIDE2 && d->ksize != 3)
            return fail(DDPM3D_EINVAL, "conv3d: the strided input mode is the 3x3x3 Downsample conv's");
        if (d->Cin % DDPM3D_CONV_CK) return fail(DDPM3D_EINVAL, "conv3d: Cin=%d not a multiple of %d", d->Cin, DDPM3D_CONV_CK);
        if (d->C1 > 0 && (d->C0 % DDPM3D_CONV_CK || (for_launch && !d->src1)))
            return fail(DDPM3D_EINVAL, "conv3d: concat needs C0 %% %d == 0 and src1", DDPM3D_CONV_CK);
        if (!aligned16(d->src0) || (d->src1 && !aligned16(d->src1)))
            return fail(DDPM3D_EINVAL, "conv3d: sources must be 16-byte aligned");
        if (d->in_mode == DDPM3D_IN_UP && ((d->H | d->W) & 1))
            return fail(DDPM3D_EINVAL, "conv3d: upsampled input needs even H, W (got %d, %d)", d->H, d->W);
    }
    if ((d->aff_a == nullptr) != (d->aff_b == nullptr)) return fail(DDPM3D_EINVAL, "conv3d: aff_a/aff_b must come together");
    if (d->aff_a && (!aligned16(d->aff_a) || !aligned16(d->aff_b)))
        return fail(DDPM3D_EINVAL, "conv3d: affine tables must be 16-byte aligned");
    if (!aligned16(d->w_packed)) return fail(DDPM3D_EINVAL, "conv3d: w_packed must be 16-byte aligned");
    if (d->res_mode < 0 || d->res_mode > 3 || (d->res_mode != DDPM3D_RES_NONE && !d->res))
        return fail(DDPM3D_EINVAL, "conv3d: residual mode %d without / with bad buffer", d->res_mode);
    if (d->res_mode == DDPM3D_RES_UP && ((d->H | d->W) & 1))
        return fail(DDPM3D_EINVAL, "conv3d: upsampled residual needs even H, W");
    if (d->bias_stride_n < 0) return fail(DDPM3D_EINVAL, "conv3d: negative bias_stride_n");
    if (d->out_layout != DDPM3D_OUT_NDHWC && d->out_layout != DDPM3D_OUT_NCDHW)
        return fail(DDPM3D_EINVAL, "conv3d: out_layout %d", d->out_layout);

    c = ddpm3d_conv_cfg(d->N, d->D, d->H, d->W, d->Cin, d->Cout, d->ksize, d->precision);
    if (d->kernel_hint & DDPM3D_HINT_SPLITK_MASK) {
        // measurements (tools/splitk_sweep.py): force the split factor; the caller sizes statistics and workspace
        // with ddpm3d_conv_plan on the same descriptor
        const int s_forced = (d->kernel_hint & DDPM3D_HINT_SPLITK_MASK) >> DDPM3D_HINT_SPLITK_SHIFT;
        const int nch = ddpm3d_cin_pad(d->Cin) / DDPM3D_CONV_CK;
        if (s_forced > nch || (s_forced != c.S && c.WN != 4))
            return fail(DDPM3D_EINVAL, "conv3d: a forced split factor needs Cout > 64 and S <= Cin / 16");
        ddpm3d_conv_cfg_split(c, s_forced, d->N, d->D, d->H, d->W, d->Cout);
    }
    if (ddpm3d_prec_wz(d->precision) &&
        !(wz_layer_ok(d->Cout, d->Cin, d->ksize) && c.WN == 4 && c.MT == 4 &&
          (d->in_mode == DDPM3D_IN_SAME || d->in_mode == DDPM3D_IN_UP)))
        return fail(DDPM3D_ENOSUP, "conv3d: the Winograd-D form needs ksize 3, Cout %% 128 == 0 "
                                   "and input mode SAME or UP; use the F16X3 packing for this call");
    if (for_launch && c.S > 1 && (!d->workspace || d->workspace_bytes < c.workspace_bytes || !aligned16(d->workspace)))
        return fail(DDPM3D_EINVAL, "conv3d: this shape is split %d-way over Cin and needs %zu bytes of "
                                   "16-byte aligned workspace (got %zu)", c.S, c.workspace_bytes,
                    d->workspace ? d->workspace_bytes : (size_t)0);
    memset(&k, 0, sizeof(k));
    k.src0 = d->src0; k.src1 = d->src1; k.affA = d->aff_a; k.affB = d->aff_b;
    k.w = (const float*)d->w_packed; k.bias = d->bias; k.res = d->res; k.out = d->out; k.stats = d->stats;
    k.N = d->N; k.D = d->D; k.H = d->H; k.W = d->W; k.Cin = d->Cin; k.Cout = d->Cout;
    k.C0 = d->C0; k.C1 = d->C1;
    k.CinPad = ddpm3d_cin_pad(d->Cin); k.CoutPad = ddpm3d_cout_pad(d->Cout);
    k.in_mode = d->in_mode; k.act = d->act; k.bias_stride_n = d->bias_stride_n;
    k.res_mode = d->res_mode; k.out_layout = d->out_layout;
    k.stats_rows = c.stats_rows;
    k.reduce_vox = c.reduce_vox;
    // DDPM3D_HINT_UP_PHASE: w_packed is the phase image; the phase form where the low-resolution grid tiles like the
    // output grid, else the shipped path on the Winograd-D image the buffer starts with (hint bit dropped)
    if ((d->kernel_hint & DDPM3D_HINT_UP_PHASE) && (d->precision != DDPM3D_PREC_F16X3_WZ || d->in_mode != DDPM3D_IN_UP))
        return fail(DDPM3D_EINVAL, "conv3d: DDPM3D_HINT_UP_PHASE needs precision F16X3_WZ and in_mode UP");
    s = ddpm3d_conv_select(*d, c, skip_cx);
    k.tilesZ = s.tilesZ; k.tilesY = s.tilesY; k.tilesX = s.tilesX;
    k.hint = s.hint;
    // the image this call reads: the phase image behind the Winograd-D one, else the buffer's (first) image
    const bool phase = s.kernel == CONV_WZ && s.variant == WZV_UP;
    const PackedImage img = phase ? ddpm3d_up_phase_image(d->Cout, d->Cin)
                                  : ddpm3d_packed_image(d->Cout, d->Cin, d->ksize, d->precision);
    k.w = (const float*)((const char*)d->w_packed + s.w_offset);
    k.io = d->io_dtype;
    if (d->io_dtype & ~(DDPM3D_IO_SRC0_BF16 | DDPM3D_IO_SRC1_BF16 | DDPM3D_IO_OUT_BF16 | DDPM3D_IO_RES_BF16 |
                        DDPM3D_IO_HALF_IS_F16))
        return fail(DDPM3D_EINVAL, "conv3d: unknown io_dtype bits %#x", d->io_dtype);
    if ((d->io_dtype & DDPM3D_IO_OUT_BF16) && d->out_layout != DDPM3D_OUT_NDHWC)
        return fail(DDPM3D_EINVAL, "conv3d: a 16-bit output needs the NDHWC layout");
    if ((d->io_dtype & (DDPM3D_IO_SRC0_BF16 | DDPM3D_IO_SRC1_BF16)) && d->in_mode == DDPM3D_IN_PLANAR2)
        return fail(DDPM3D_EINVAL, "conv3d: the planar input volumes are fp32");
    if (prec_scaled(d->precision)) {
        if (!d->in_bound || d->in_bound_count <= 0 || d->in_bound_count > 64 || d->in_bound_stride <= 0)
            return fail(DDPM3D_EINVAL, "conv3d: the split-f16 precisions need in_bound (1..64 entries per sample): "
                                       "the activation scale is derived from it, nothing is clamped");
        k.in_bound = d->in_bound;
        k.in_bound_count = d->in_bound_count;
        k.in_bound_stride = d->in_bound_stride;
    }
    k.ksplit = c.S;
    k.chunks_per_split = (k.CinPad / DDPM3D_CONV_CK + c.S - 1) / c.S;
    // 1x1 convs: whole 32-channel blocks per split (conv1x1.hip walks K in those; any range suits the general kernel)
    if (d->ksize == 1 && c.S > 1) k.chunks_per_split = (k.chunks_per_split + 1) & ~1;
    k.partial = (float*)d->workspace;
    {
        // extents for the kernel's buffer descriptors (32-bit offsets)
        const bool dbl = d->in_mode == DDPM3D_IN_POOL || d->in_mode == DDPM3D_IN_STRIDE2;
        const long long Hs = dbl ? 2LL * d->H : (d->in_mode == DDPM3D_IN_UP ? d->H / 2 : d->H);
        const long long Ws = dbl ? 2LL * d->W : (d->in_mode == DDPM3D_IN_UP ? d->W / 2 : d->W);
        const long long vox = (long long)d->N * d->D * Hs * Ws;
        const long long b0 = vox * d->C0 * ((d->io_dtype & DDPM3D_IO_SRC0_BF16) ? 2 : 4);
        const long long b1 = vox * d->C1 * ((d->io_dtype & DDPM3D_IO_SRC1_BF16) ? 2 : 4);
        const size_t wb = phase ? img.body : img.bytes();
        if (b0 >= 0xFFFFFFF0LL || b1 >= 0xFFFFFFF0LL || wb >= 0xFFFFFFF0ULL)
            return fail(DDPM3D_E2BIG, "conv3d: a source tensor or the weights exceed 4 GiB; split the batch");
        // the epilogue addresses one SAMPLE of the output (or residual) with 32-bit offsets
        if ((long long)d->D * d->H * d->W * d->Cout * 4 >= 0xFFFFFFF0LL)
            return fail(DDPM3D_E2BIG, "conv3d: one output sample exceeds 4 GiB; tile the volume");
        k.src0_bytes = (unsigned)b0; k.src1_bytes = (unsigned)b1; k.w_bytes = (unsigned)wb;
        // workgroup -> XCD order: keep on one XCD whichever operand is the larger stream
        k.wstat = (d->kernel_hint & DDPM3D_HINT_WSTAT_ON)    ? 1
                  : (d->kernel_hint & DDPM3D_HINT_WSTAT_OFF) ? 0
                                                             : ((long long)wb > b0 + b1 ? 1 : 0);
    }
    if (img.scales) k.wscale = (const float*)((const char*)k.w + img.body);  // output scales sit behind the taps
    if (d->stats && d->stats_rows != k.stats_rows)
        return fail(DDPM3D_EINVAL, "conv3d: stats_rows=%d, this shape writes %d", d->stats_rows, k.stats_rows);
    if (d->stats && !aligned16(d->stats)) return fail(DDPM3D_EINVAL, "conv3d: stats must be 16-byte aligned");
    if (d->stats && d->out_layout != DDPM3D_OUT_NDHWC)
        return fail(DDPM3D_EINVAL, "conv3d: statistics only with NDHWC output");
    const long long blocks = (long long)k.N * c.tilesZ * c.tilesY * c.tilesX;    // (the tiles the shape rule counted)
    if (blocks > 0x7fffffffLL) return fail(DDPM3D_EINVAL, "conv3d: grid too large");
    return DDPM3D_OK;
}

int ddpm3d_conv3d(const ddpm3d_conv_desc* d, void* stream) {
    ConvK k;
    ConvCfg c;
    ConvSel s;
    const int ok = conv_prepare(d, k, c, s, true);
    if (ok != DDPM3D_OK) return ok;
    const int rc = launched(ddpm3d_launch_conv(k, s, (hipStream_t)stream),
                            s.kernel == CONV_SKINNY ? "conv3d (skinny)" : s.kernel == CONV_PW ? "conv3d (1x1)" : "conv3d");
    if (rc != DDPM3D_OK || c.S == 1) return rc;
    return launched(ddpm3d_launch_splitk_reduce(k, (hipStream_t)stream), "conv3d split-K reduce");
}

// ---- ddpm3d_conv3d_skip: out = conv2(act(A h + B)) + skip(x) + biases, the tail of a ResBlock whose skip connection is a
// 1x1 conv (unet.py:173-186, :256).  Validation shared by the entry and its query: fills the skip conv's own descriptor
// (the two-step form's first call), conv2's launch record with the sk_* fields, and says whether the fused form runs.
static int base_prec(int p) {
    return p == DDPM3D_PREC_F16X3_WZ ? DDPM3D_PREC_F16X3 : p == DDPM3D_PREC_F16_WZ ? DDPM3D_PREC_F16
         : p == DDPM3D_PREC_BF16_WZ ? DDPM3D_PREC_BF16 : p;
}
static int skip_prepare(const ddpm3d_conv_desc* d, const ddpm3d_conv_skip* sk, ddpm3d_conv_desc& sd, ConvK& k, ConvCfg& c,
                        ConvSel& s, bool& fused, bool for_launch) {
    fused = false;
    if (!d || !sk) return fail(DDPM3D_EINVAL, "conv3d_skip: null descriptor");
    if (d->res_mode != DDPM3D_RES_NONE || d->res)
        return fail(DDPM3D_EINVAL, "conv3d_skip: conv2 carries no residual of its own (the skip conv is its residual)");
    if (d->out_layout != DDPM3D_OUT_NDHWC) return fail(DDPM3D_EINVAL, "conv3d_skip: NDHWC output only");
    if (d->ksize != 3) return fail(DDPM3D_EINVAL, "conv3d_skip: conv2 is a 3x3x3 conv (ksize %d)", d->ksize);
    if (sk->C0 <= 0 || sk->C1 < 0) return fail(DDPM3D_EINVAL, "conv3d_skip: C0=%d C1=%d", sk->C0, sk->C1);
    if (sk->io_dtype & ~(DDPM3D_IO_SRC0_BF16 | DDPM3D_IO_SRC1_BF16))
        return fail(DDPM3D_EINVAL, "conv3d_skip: skip io_dtype names sources only (%#x)", sk->io_dtype);
    memset(&sd, 0, sizeof(sd));
    sd.N = d->N; sd.D = d->D; sd.H = d->H; sd.W = d->W;
    sd.C0 = sk->C0; sd.C1 = sk->C1; sd.Cin = sk->C0 + sk->C1; sd.Cout = d->Cout;
    sd.ksize = 1; sd.in_mode = DDPM3D_IN_SAME;
    sd.src0 = sk->src0; sd.src1 = sk->src1;
    sd.act = DDPM3D_ACT_NONE; sd.precision = base_prec(d->precision);
    sd.w_packed = sk->w_packed; sd.bias = sk->bias;
    sd.res_mode = DDPM3D_RES_NONE;
    sd.out = d->out; sd.out_layout = DDPM3D_OUT_NDHWC;
    sd.workspace = d->workspace; sd.workspace_bytes = d->workspace_bytes;
    sd.in_bound = sk->in_bound; sd.in_bound_count = sk->in_bound_count; sd.in_bound_stride = sk->in_bound_stride;
    sd.io_dtype = sk->io_dtype | (d->io_dtype & (DDPM3D_IO_OUT_BF16 | DDPM3D_IO_HALF_IS_F16));
    ConvK ks;
    ConvCfg cs;
    ConvSel ss;
    int ok = conv_prepare(&sd, ks, cs, ss, false);
    if (ok != DDPM3D_OK) return ok;
    if (for_launch && (!sk->src0 || !sk->w_packed || !sk->bias)) return fail(DDPM3D_EINVAL, "conv3d_skip: null buffer");
    // the fused form exists for: f16x3 Winograd-D conv2 on a plain fp32 input, the default issue order; a skip conv that
    // conv1x1.hip would take (whole 32-channel blocks), fp32 tensors throughout.  Whether such a pair runs it is
    // ddpm3d_conv_select's decision (the measured rule)
    const int cand = d->precision == DDPM3D_PREC_F16X3_WZ && d->in_mode == DDPM3D_IN_SAME && d->io_dtype == 0 &&
                     sk->io_dtype == 0 && !(d->kernel_hint & (DDPM3D_HINT_UP_PHASE | DDPM3D_HINT_WZ_ORDER_MASK)) &&
                     ss.kernel == CONV_PW && aligned16(sk->bias);
    ok = conv_prepare(d, k, c, s, for_launch && cand, cand ? sd.Cin : 0);
    if (ok != DDPM3D_OK) return ok;
    fused = s.kernel == CONV_WZ && s.variant == WZV_SKIP;
    if (!fused) return DDPM3D_OK;
    k.sk_src0 = sk->src0; k.sk_src1 = sk->src1; k.sk_C0 = sk->C0; k.sk_C1 = sk->C1;
    k.sk_src0_bytes = ks.src0_bytes; k.sk_src1_bytes = ks.src1_bytes;
    k.sk_w = ks.w; k.sk_w_bytes = ks.w_bytes; k.sk_wscale = ks.wscale;
    k.sk_bias = sk->bias;
    k.sk_bound = sk->in_bound; k.sk_bound_count = sk->in_bound_count; k.sk_bound_stride = sk->in_bound_stride;
    k.sk_blocks_per_split = (sd.Cin / 32 + c.S - 1) / c.S;
    return DDPM3D_OK;
}

int ddpm3d_conv3d_skip(const ddpm3d_conv_desc* d, const ddpm3d_conv_skip* sk, void* stream) {
    ddpm3d_conv_desc sd;
    ConvK k;
    ConvCfg c;
    ConvSel s;
    bool fused = false;
    const int ok = skip_prepare(d, sk, sd, k, c, s, fused, true);
    if (ok != DDPM3D_OK) return ok;
    if (fused) {
        const int rc = launched(ddpm3d_launch_conv(k, s, (hipStream_t)stream), "conv3d_skip");
        if (rc != DDPM3D_OK || c.S == 1) return rc;
        return launched(ddpm3d_launch_splitk_reduce(k, (hipStream_t)stream), "conv3d_skip split-K reduce");
    }
    // today's two steps: the 1x1 conv into out, then conv2 with out as its same-shape residual
    const int rc = ddpm3d_conv3d(&sd, stream);
    if (rc != DDPM3D_OK) return rc;
    ddpm3d_conv_desc d2 = *d;
    d2.res = d->out;
    d2.res_mode = DDPM3D_RES_SAME;
    if (d->io_dtype & DDPM3D_IO_OUT_BF16) d2.io_dtype |= DDPM3D_IO_RES_BF16;
    return ddpm3d_conv3d(&d2, stream);
}

int ddpm3d_conv_skip_fused(const ddpm3d_conv_desc* d, const ddpm3d_conv_skip* sk) {
    ddpm3d_conv_desc sd;
    ConvK k;
    ConvCfg c;
    ConvSel s;
    bool fused = false;
    return skip_prepare(d, sk, sd, k, c, s, fused, false) == DDPM3D_OK && fused ? 1 : 0;
}

int ddpm3d_conv_plan(const ddpm3d_conv_desc* d, int* stats_rows, size_t* workspace_bytes, int* split) {
    ConvK k;
    ConvCfg c;
    ConvSel s;
    const int ok = conv_prepare(d, k, c, s, false);
    if (ok != DDPM3D_OK) return ok;
    if (stats_rows) *stats_rows = c.stats_rows;
    if (workspace_bytes) *workspace_bytes = c.workspace_bytes;
    if (split) *split = c.S;
    return DDPM3D_OK;
}

int ddpm3d_conv_kernel_family(const ddpm3d_conv_desc* d, char* name, int name_len) {
    if (!name || name_len <= 0) return fail(DDPM3D_EINVAL, "conv_kernel_family: no buffer");
    ConvK k;
    ConvCfg c;
    ConvSel s;
    const int ok = conv_prepare(d, k, c, s, false);   // (the split-K workspace may be attached later)
    if (ok != DDPM3D_OK) return ok;
    const int tile = 1 << c.TXL;    // 8: 8x8x2 / 8x4x4 tiles, 4: 4x4x8
    int n;
    if (s.kernel == CONV_SKINNY) n = snprintf(name, (size_t)name_len, "conv3d_p%d_k3_skinny", d->precision);
    else if (s.kernel == CONV_PW) n = snprintf(name, (size_t)name_len, "conv1x1_p%d_t%d", d->precision, tile);
    else n = snprintf(name, (size_t)name_len, "conv3d_p%d_k%d_wn%d_t%d", d->precision, d->ksize, c.WN, tile);
    if (n < 0 || n >= name_len) return fail(DDPM3D_EINVAL, "conv_kernel_family: buffer of %d bytes is too short", name_len);
    return DDPM3D_OK;
}

int ddpm3d_conv_kernel_instance(const ddpm3d_conv_desc* d, const ddpm3d_conv_skip* sk, char* name, int name_len) {
    if (!name || name_len <= 0) return fail(DDPM3D_EINVAL, "conv_kernel_instance: no buffer");
    ddpm3d_conv_desc sd;
    ConvK k;
    ConvCfg c;
    ConvSel s;
    bool fused = false;
    int ok = sk ? skip_prepare(d, sk, sd, k, c, s, fused, false) : conv_prepare(d, k, c, s, false);
    if (ok == DDPM3D_OK && sk && !fused) {
        // two calls: conv2 as the entry issues it, with the 1x1 conv's output as its residual
        static const float unattached = 0.0f;
        ddpm3d_conv_desc d2 = *d;
        d2.res = d->out ? d->out : &unattached;
        d2.res_mode = DDPM3D_RES_SAME;
        if (d->io_dtype & DDPM3D_IO_OUT_BF16) d2.io_dtype |= DDPM3D_IO_RES_BF16;
        ok = conv_prepare(&d2, k, c, s, false);
    }
    if (ok != DDPM3D_OK) return ok;
    const int n = ddpm3d_conv_sel_name(s, name, (size_t)name_len);
    if (n < 0 || n >= name_len) return fail(DDPM3D_EINVAL, "conv_kernel_instance: buffer of %d bytes is too short", name_len);
    return DDPM3D_OK;
}

int ddpm3d_gn_finalize(const double* stats0, int C0, int rows0, const double* stats1, int C1, int rows1,
                       int N, int groups, double count, float eps, const float* gamma, const float* beta,
                       const float* film, int film_stride, int film_off, float* aff_a, float* aff_b,
                       float* bound, void* stream) {
    const int C = C0 + C1;
    if (!stats0 || N <= 0 || groups <= 0 || C0 <= 0 || C1 < 0 || rows0 <= 0 || count <= 0)
        return fail(DDPM3D_EINVAL, "gn_finalize: bad arguments");
    if (!aligned16(stats0) || (stats1 && !aligned16(stats1)))
        return fail(DDPM3D_EINVAL, "gn_finalize: statistics must be 16-byte aligned");
    if (gamma ? (!beta || !aff_a || !aff_b) : !bound)
        return fail(DDPM3D_EINVAL, "gn_finalize: gamma needs beta, aff_a, aff_b; without gamma only `bound` is written");
    if (C % groups) return fail(DDPM3D_EINVAL, "gn_finalize: C=%d not divisible by %d groups", C, groups);
    const int cg = C / groups;
    if (C1 > 0 && (!stats1 || rows1 <= 0 || C0 % cg))
        return fail(DDPM3D_EINVAL, "gn_finalize: a group straddles the concat boundary (C0=%d, group=%d)", C0, cg);
    return launched(ddpm3d_launch_gn_finalize(stats0, C0, rows0, stats1, C1, rows1, N, groups, count, eps,
                                              gamma, beta, film, film_stride, film_off, aff_a, aff_b, bound,
                                              (hipStream_t)stream),
                    "gn_finalize");
}

int ddpm3d_absmax(const float* x0, const float* x1, int N, size_t per_sample, float* bound, void* stream) {
    if (!x0 || !bound || N <= 0 || per_sample == 0) return fail(DDPM3D_EINVAL, "absmax: bad arguments");
    return launched(ddpm3d_launch_absmax(x0, x1, N, per_sample, bound, (hipStream_t)stream), "absmax");
}

int ddpm3d_gn_stats_rows(int voxels) { return voxels > 0 ? ddpm3d_gn_stats_rows_impl(voxels) : 0; }

int ddpm3d_gn_stats(const float* x, int N, int voxels, int C, double* stats, void* stream) {
    if (!x || !stats || N <= 0 || voxels <= 0 || C <= 0 || (C & 3) || !aligned16(x) || !aligned16(stats))
        return fail(DDPM3D_EINVAL, "gn_stats: bad arguments (C must be a multiple of 4, x 16-byte aligned)");
    return launched(ddpm3d_launch_gn_stats(x, N, voxels, C, stats, (hipStream_t)stream), "gn_stats");
}

int ddpm3d_timestep_embedding(const float* t, int rows, int dim, const float* freqs, float* out, void* stream) {
    if (!t || !out || !freqs || rows <= 0 || dim <= 1) return fail(DDPM3D_EINVAL, "timestep_embedding: bad arguments");
    return launched(ddpm3d_launch_timestep_embedding(t, rows, dim, freqs, out, (hipStream_t)stream),
                    "timestep_embedding");
}

int ddpm3d_linear(const float* in, int rows, int K, const float* w, const float* bias, int O, int silu_in,
                  float* out, int out_stride, void* stream) {
    if (!in || !w || !bias || !out || rows <= 0 || K <= 0 || O <= 0 || out_stride < O)
        return fail(DDPM3D_EINVAL, "linear: bad arguments");
    return launched(ddpm3d_launch_linear(in, rows, K, w, bias, O, silu_in, out, out_stride, (hipStream_t)stream),
                    "linear");
}

int ddpm3d_pool_act(const void* src, const float* aff_a, const float* aff_b, int act, int fast_act, int N, int D,
                    int H, int W, int C, void* out, int io_dtype, void* stream) {
    if (!src || !out || N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3))
        return fail(DDPM3D_EINVAL, "pool_act: bad arguments (C must be a multiple of 4)");
    if ((aff_a == nullptr) != (aff_b == nullptr)) return fail(DDPM3D_EINVAL, "pool_act: aff_a/aff_b must come together");
    if (act && !aff_a) return fail(DDPM3D_EINVAL, "pool_act: an activation needs the affine tables (pass A = 1, B = 0)");
    if (io_dtype & ~(DDPM3D_IO_SRC0_BF16 | DDPM3D_IO_OUT_BF16 | DDPM3D_IO_HALF_IS_F16))
        return fail(DDPM3D_EINVAL, "pool_act: io_dtype bits %#x", io_dtype);
    if (!aligned16(src) || !aligned16(out) || (aff_a && (!aligned16(aff_a) || !aligned16(aff_b))))
        return fail(DDPM3D_EINVAL, "pool_act: buffers must be 16-byte aligned");
    if ((long long)N * D * H * W * (C / 4) > 0x7fffffffLL * 256)
        return fail(DDPM3D_E2BIG, "pool_act: grid too large; split the batch");
    return launched(ddpm3d_launch_pool_act((const float*)src, aff_a, aff_b, act, fast_act, N, D, H, W, C, (float*)out,
                                           (io_dtype & DDPM3D_IO_SRC0_BF16) != 0, (io_dtype & DDPM3D_IO_OUT_BF16) != 0,
                                           (io_dtype & DDPM3D_IO_HALF_IS_F16) != 0, (hipStream_t)stream),
                    "pool_act");
}

int ddpm3d_add_embedding(float* emb, const float* table, const int64_t* idx, int rows, int dim, int num_classes,
                         void* stream) {
    if (!emb || !table || !idx || rows <= 0 || dim <= 0 || num_classes <= 0)
        return fail(DDPM3D_EINVAL, "add_embedding: bad arguments");
    return launched(ddpm3d_launch_add_embedding(emb, table, idx, rows, dim, num_classes, (hipStream_t)stream), "add_embedding");
}

int ddpm3d_ncdhw_to_ndhwc(const float* in, int N, int C, int voxels, float* out, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || voxels <= 0) return fail(DDPM3D_EINVAL, "ncdhw_to_ndhwc: bad arguments");
    return launched(ddpm3d_launch_transpose(in, N, C, voxels, out, (hipStream_t)stream), "ncdhw_to_ndhwc");
}
int ddpm3d_ndhwc_to_ncdhw(const float* in, int N, int C, int voxels, float* out, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || voxels <= 0) return fail(DDPM3D_EINVAL, "ndhwc_to_ncdhw: bad arguments");
    return launched(ddpm3d_launch_transpose(in, N, voxels, C, out, (hipStream_t)stream), "ndhwc_to_ncdhw");
}

int ddpm3d_ncdhw_to_ndhwc_pad(const float* in, int N, int C, int voxels, int Cpad, float* out, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || voxels <= 0 || Cpad < C)
        return fail(DDPM3D_EINVAL, "ncdhw_to_ndhwc_pad: bad arguments");
    return launched(ddpm3d_launch_to_ndhwc_pad(in, N, C, voxels, Cpad, out, (hipStream_t)stream), "ncdhw_to_ndhwc_pad");
}

int ddpm3d_subsample_hw2(const float* in, int N, int D, int H, int W, int C, float* out, void* stream) {
    if (!in || !out || N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || (H & 1) || (W & 1) || (C & 3) ||
        !aligned16(in) || !aligned16(out))
        return fail(DDPM3D_EINVAL, "subsample_hw2: needs even H, W, C %% 4 == 0 and 16-byte aligned tensors");
    return launched(ddpm3d_launch_subsample_hw2(in, N, D, H, W, C, out, (hipStream_t)stream), "subsample_hw2");
}

int ddpm3d_attention_p(const float* qkv, int N, int T, int heads, int head_channels, int precision,
                       const float* qkv_bound, int bound_count, int bound_stride, float* out, void* stream) {
    if (!qkv || !out || N <= 0 || T <= 0 || heads <= 0) return fail(DDPM3D_EINVAL, "attention: bad arguments");
    if (head_channels != 32 && head_channels != 64 && head_channels != 128)
        return fail(DDPM3D_ENOSUP, "attention: %d channels per head (32, 64 or 128 are built)", head_channels);
    if (precision != DDPM3D_PREC_F32 && precision != DDPM3D_PREC_F16X3)
        return fail(DDPM3D_ENOSUP, "attention: precision %d (F32 and F16X3 are built)", precision);
    if (!aligned16(qkv) || !aligned16(out)) return fail(DDPM3D_EINVAL, "attention: buffers must be 16-byte aligned");
    if (precision != DDPM3D_PREC_F32 && (!qkv_bound || bound_count <= 0 || bound_count > 64 || bound_stride <= 0))
        return fail(DDPM3D_EINVAL, "attention: the split-f16 arithmetic needs qkv_bound (1..64 entries per sample)");
    return launched(ddpm3d_launch_attention(qkv, N, T, heads, head_channels, precision, qkv_bound, bound_count,
                                            bound_stride, out, (hipStream_t)stream),
                    "attention");
}

int ddpm3d_attention(const float* qkv, int N, int T, int heads, int head_channels, float* out, void* stream) {
    return ddpm3d_attention_p(qkv, N, T, heads, head_channels, DDPM3D_PREC_F32, nullptr, 0, 0, out, stream);
}

// ------------------------------------------------------------ variational bound
// grid.y carries the sample index of the element-wise launches
static bool vb_shape_ok(int N, int voxels, int T) { return N > 0 && N <= 65535 && voxels > 0 && T > 0; }

// flags are the sampler's
static const int STEP_FLAGS = DDPM3D_F_LEARN_SIGMA | DDPM3D_F_PREDICT_XSTART | DDPM3D_F_CLIP;

// The checks the step entries that take T share: the entry's own pointer checks (ptrs_ok) and the shape, then the
// flags.  Entry-specific checks follow it.
static int step_entry_ok(const char* what, bool ptrs_ok, int N, int voxels, int T, int flags) {
    if (!ptrs_ok || !vb_shape_ok(N, voxels, T))
        return fail(DDPM3D_EINVAL, "%s: bad arguments (N=%d voxels=%d T=%d)", what, N, voxels, T);
    if (flags & ~STEP_FLAGS) return fail(DDPM3D_EINVAL, "%s: unknown flag bits %#x", what, flags);
    return DDPM3D_OK;
}

int ddpm3d_q_sample(const float* x_start, const float* noise, const float* qcoef, const int64_t* t_idx, int N,
                    int voxels, int T, float* x_t, void* stream) {
    if (!x_start || !noise || !qcoef || !t_idx || !x_t || !vb_shape_ok(N, voxels, T))
        return fail(DDPM3D_EINVAL, "q_sample: bad arguments (N=%d voxels=%d T=%d)", N, voxels, T);
    return launched(ddpm3d_launch_q_sample(x_start, noise, nullptr, qcoef, t_idx, N, voxels, T, x_t, (hipStream_t)stream),
                    "q_sample");
}

size_t ddpm3d_vb_terms_workspace_bytes(int N, int voxels) {
    if (N <= 0 || voxels <= 0) return 0;
    return (size_t)N * (size_t)ddpm3d_vb_parts(voxels) * 4 * sizeof(double);
}

// the one workspace check of every entry that takes a caller's workspace of `need` bytes
static int ws_ok(const char* what, size_t need, const void* ws, size_t ws_bytes) {
    if (!ws || ws_bytes < need || !aligned16(ws))
        return fail(DDPM3D_EINVAL, "%s: needs %zu bytes of 16-byte aligned workspace (got %zu)", what, need,
                    ws ? ws_bytes : (size_t)0);
    return DDPM3D_OK;
}

int ddpm3d_vb_terms(const float* model_out, const float* x_start, const float* x_t, const float* noise,
                    const float* coef, const float* qcoef, const int64_t* t_idx, int N, int voxels, int T,
                    int flags, void* ws, size_t ws_bytes, float* vb, float* xstart_mse, float* mse, int ld_out,
                    float* pred_xstart, void* stream) {
    // its bad-arguments message reports ld_out too, so step_entry_ok adds only the flag check here
    if (!model_out || !x_start || !x_t || !coef || !qcoef || !t_idx || !vb || !vb_shape_ok(N, voxels, T) ||
        ld_out <= 0)
        return fail(DDPM3D_EINVAL, "vb_terms: bad arguments (N=%d voxels=%d T=%d ld_out=%d)", N, voxels, T, ld_out);
    if ((noise == nullptr) != (mse == nullptr))
        return fail(DDPM3D_EINVAL, "vb_terms: noise and mse must come together");
    int rc = step_entry_ok("vb_terms", true, N, voxels, T, flags);
    if (rc == DDPM3D_OK) rc = ws_ok("vb_terms", ddpm3d_vb_terms_workspace_bytes(N, voxels), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_vb_terms(model_out, x_start, x_t, noise, coef, qcoef, t_idx, N, voxels, T, flags,
                                           (double*)ws, vb, xstart_mse, mse, ld_out, pred_xstart,
                                           (hipStream_t)stream),
                    "vb_terms");
}

int ddpm3d_prior_bpd(const float* x_start, const float* qcoef, int N, int voxels, int T, void* ws, size_t ws_bytes,
                     float* out, void* stream) {
    if (!x_start || !qcoef || !out || !vb_shape_ok(N, voxels, T))
        return fail(DDPM3D_EINVAL, "prior_bpd: bad arguments (N=%d voxels=%d T=%d)", N, voxels, T);
    const int rc = ws_ok("prior_bpd", ddpm3d_vb_terms_workspace_bytes(N, voxels), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_prior_bpd(x_start, qcoef, N, voxels, T, (double*)ws, out, (hipStream_t)stream),
                    "prior_bpd");
}

// ------------------------------------------------- p_mean_variance, DDIM inversion (added within ABI 13)

int ddpm3d_p_mean_variance(const float* model_out, const float* x, const float* coef, const int64_t* t_idx, int N,
                           int voxels, int T, int flags, float* mean, float* variance, float* log_variance,
                           float* pred_xstart, void* stream) {
    const int rc = step_entry_ok("p_mean_variance", model_out && x && coef && t_idx && mean && pred_xstart, N, voxels,
                                 T, flags);
    if (rc != DDPM3D_OK) return rc;
    if (flags & DDPM3D_F_LEARN_SIGMA) {
        if (!variance || !log_variance)
            return fail(DDPM3D_EINVAL, "p_mean_variance: F_LEARN_SIGMA needs variance and log_variance");
    } else if (variance || log_variance) {
        return fail(DDPM3D_EINVAL, "p_mean_variance: variance and log_variance must be NULL without F_LEARN_SIGMA");
    }
    return launched(ddpm3d_launch_p_mean_variance(model_out, x, coef, t_idx, N, voxels, T, flags, mean, variance,
                                                  log_variance, pred_xstart, (hipStream_t)stream),
                    "p_mean_variance");
}

int ddpm3d_ddim_reverse_step(const float* model_out, const float* x, const float* coef, const int64_t* t_idx, int N,
                             int voxels, int T, int flags, float* sample, float* pred_xstart, void* stream) {
    const int rc = step_entry_ok("ddim_reverse_step", model_out && x && coef && t_idx && sample, N, voxels, T, flags);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_ddim_reverse_step(model_out, x, coef, t_idx, N, voxels, T, flags, sample,
                                                    pred_xstart, (hipStream_t)stream),
                    "ddim_reverse_step");
}

// ------------------------------------------------- sampler noise from a counter-based key (added within ABI 13)
// The host side of a key; `geometry`: the entry reads origin / patch / canvas (ddpm3d_noise_bits does not).
static int noise_key_ok(const char* what, const ddpm3d_noise_key* key, int N, int voxels, bool geometry) {
    if (!key || !key->stream) return fail(DDPM3D_EINVAL, "%s: NULL key or key->stream", what);
    if (N <= 0 || N > 65535 || voxels <= 0)
        return fail(DDPM3D_EINVAL, "%s: bad arguments (N=%d voxels=%d)", what, N, voxels);
    if (key->draw < 0 || key->draw > 0xffffffffll)
        return fail(DDPM3D_EINVAL, "%s: draw %lld outside 0 .. 2^32 - 1", what, (long long)key->draw);
    if (geometry && key->origin) {
        for (int a = 0; a < 3; ++a)
            if (key->patch[a] <= 0 || key->canvas[a] <= 0)
                return fail(DDPM3D_EINVAL, "%s: patch (%d, %d, %d) and canvas (%d, %d, %d) extents must be positive",
                            what, key->patch[0], key->patch[1], key->patch[2], key->canvas[0], key->canvas[1],
                            key->canvas[2]);
        // three factors below 2^31 each: the partial products fit 64 bits only after the first check
        const uint64_t LIMIT = 1ull << 34;
        const uint64_t p01 = (uint64_t)key->patch[0] * (uint64_t)key->patch[1];
        if (p01 > (uint64_t)voxels || p01 * (uint64_t)key->patch[2] != (uint64_t)voxels)
            return fail(DDPM3D_EINVAL, "%s: patch %d x %d x %d is not voxels=%d", what, key->patch[0], key->patch[1],
                        key->patch[2], voxels);
        const uint64_t c01 = (uint64_t)key->canvas[0] * (uint64_t)key->canvas[1];
        if (c01 > LIMIT || c01 * (uint64_t)key->canvas[2] > LIMIT)
            return fail(DDPM3D_EINVAL, "%s: canvas %d x %d x %d holds more than 2^34 voxels", what, key->canvas[0],
                        key->canvas[1], key->canvas[2]);
    }
    return DDPM3D_OK;
}

int ddpm3d_noise_fill(const ddpm3d_noise_key* key, int N, int voxels, float* out, void* stream) {
    const int rc = noise_key_ok("noise_fill", key, N, voxels, true);
    if (rc != DDPM3D_OK) return rc;
    if (!out) return fail(DDPM3D_EINVAL, "noise_fill: NULL out");
    return launched(ddpm3d_launch_noise_fill(*key, N, voxels, out, (hipStream_t)stream), "noise_fill");
}

int ddpm3d_noise_bits(const ddpm3d_noise_key* key, int N, int quads, uint32_t* out, void* stream) {
    const int rc = noise_key_ok("noise_bits", key, N, quads, false);
    if (rc != DDPM3D_OK) return rc;
    if (!out) return fail(DDPM3D_EINVAL, "noise_bits: NULL out");
    return launched(ddpm3d_launch_noise_bits(*key, N, quads, out, (hipStream_t)stream), "noise_bits");
}

// ------------------------------------------------- the nine step entries
// ddpm3d_{p_sample,ddim,dpm_solver}_step{,_keyed,_x0}: one validate-and-launch function; each entry states its name,
// kind and argument style and passes its arguments in the order of the widest list (dpm_solver_step_x0's, eta after
// order), NULL or 0 for what it does not take.  The three styles keep the checks, their order and their messages of
// the ABI steps that added them: the keyed entries check the key first, the x0 entries last.
enum StepKind { STEP_DDPM, STEP_DDIM, STEP_SOLVER };
enum StepStyle { STEP_PLAIN, STEP_KEYED, STEP_X0 };
struct StepArgs {
    const float *model_out, *xstart, *x, *x0_prev1, *x0_prev2, *noise;
    const ddpm3d_noise_key* key;
    const float *coef, *scoef;
    const int64_t* t_idx;
    int N, voxels, T, flags, order;
    float eta;
    float *sample, *pred_xstart;
    void* stream;
};

static int step_entry(const char* name, StepKind kind, StepStyle style, const StepArgs& a) {
    const bool solver = kind == STEP_SOLVER;
    // the keyed solver entry names itself in its key check only: everything else it shares with the un-keyed entry,
    // under that entry's name
    const char* what = solver && style == STEP_KEYED ? "dpm_solver_step" : name;
    if (style == STEP_KEYED && (a.key || !solver)) {            // the solver's NULL key is the ODE form
        const int rc = noise_key_ok(name, a.key, a.N, a.voxels, true);
        if (rc != DDPM3D_OK) return rc;
    }
    if (style == STEP_X0) {
        // the pointers, the shape, the flags, the noise source, then the outputs apart from each other and from what is read
        if (!a.xstart || !a.x || !a.coef || !a.t_idx || !a.sample) return fail(DDPM3D_EINVAL, "%s: null pointer", what);
        if (a.N < 1 || a.N > 65535 || a.voxels < 1)
            return fail(DDPM3D_EINVAL, "%s: bad arguments (N=%d voxels=%d)", what, a.N, a.voxels);
        if (a.flags & ~STEP_FLAGS) return fail(DDPM3D_EINVAL, "%s: unknown flag bits %#x", what, a.flags);
        if (kind == STEP_DDPM && (a.flags & DDPM3D_F_LEARN_SIGMA) && !a.model_out)
            return fail(DDPM3D_EINVAL, "%s: F_LEARN_SIGMA reads model_out's second half: model_out is NULL", what);
        if (a.noise && a.key)
            return fail(DDPM3D_EINVAL, "%s: noise and key both name the noise: one of them must be NULL", what);
        if (!a.noise && !a.key && !solver) return fail(DDPM3D_EINVAL, "%s: one of noise and key must be given", what);
        const float *s = a.sample, *p = a.pred_xstart;
        if (s == p || s == a.xstart || s == a.x || s == a.noise || s == a.model_out ||
            (p && (p == a.xstart || p == a.x || p == a.noise || p == a.model_out)))
            return fail(DDPM3D_EINVAL, "%s: sample and pred_xstart must be tensors of their own", what);
        if (a.key) {
            const int rc = noise_key_ok(what, a.key, a.N, a.voxels, true);
            if (rc != DDPM3D_OK) return rc;
        }
        if (solver && (!a.scoef || !a.pred_xstart || a.T < 1))
            return fail(DDPM3D_EINVAL, "%s: bad arguments (scoef, pred_xstart or T=%d)", what, a.T);
    } else if (solver) {
        const int rc = step_entry_ok(what, a.model_out && a.x && a.coef && a.scoef && a.t_idx && a.sample && a.pred_xstart,
                                     a.N, a.voxels, a.T, a.flags);
        if (rc != DDPM3D_OK) return rc;
    } else if (!(a.model_out && a.x && (a.noise || style == STEP_KEYED) && a.coef && a.t_idx && a.sample && a.N > 0 &&
                 a.voxels > 0)) {
        return fail(DDPM3D_EINVAL, "%s: bad arguments", what);
    }
    if (!solver)
        return launched(ddpm3d_launch_sample_step(kind == STEP_DDIM, a.model_out, a.xstart, a.x, a.noise, a.key, a.coef,
                                                  a.t_idx, a.N, a.voxels, a.flags, a.eta, a.sample, a.pred_xstart,
                                                  (hipStream_t)a.stream),
                        what);
    if (a.order < 1 || a.order > 3) return fail(DDPM3D_EINVAL, "%s: order %d is not 1, 2 or 3", what, a.order);
    if ((a.order >= 2 && !a.x0_prev1) || (a.order == 3 && !a.x0_prev2))
        return fail(DDPM3D_EINVAL, "%s: order %d needs %d earlier x0 predictions", what, a.order, a.order - 1);
    if (style == STEP_X0 && (a.sample == a.x0_prev1 || a.sample == a.x0_prev2 || a.pred_xstart == a.x0_prev1 ||
                             a.pred_xstart == a.x0_prev2))
        return fail(DDPM3D_EINVAL, "%s: sample and pred_xstart must be tensors of their own", what);
    return launched(ddpm3d_launch_dpm_solver_step(a.model_out, a.xstart, a.x, a.x0_prev1, a.x0_prev2, a.noise, a.key,
                                                  a.coef, a.scoef, a.t_idx, a.N, a.voxels, a.T, a.flags, a.order,
                                                  a.sample, a.pred_xstart, (hipStream_t)a.stream),
                    what);
}

int ddpm3d_p_sample_step(const float* model_out, const float* x, const float* noise, const float* coef,
                         const int64_t* t_idx, int N, int voxels, int flags, float* sample,
                         float* pred_xstart, void* stream) {
    return step_entry("p_sample_step", STEP_DDPM, STEP_PLAIN,
                      {model_out, nullptr, x, nullptr, nullptr, noise, nullptr, coef, nullptr, t_idx, N, voxels, 0, flags,
                       0, 0.0f, sample, pred_xstart, stream});
}

int ddpm3d_ddim_step(const float* model_out, const float* x, const float* noise, const float* coef,
                     const int64_t* t_idx, int N, int voxels, int flags, float eta, float* sample,
                     float* pred_xstart, void* stream) {
    return step_entry("ddim_step", STEP_DDIM, STEP_PLAIN,
                      {model_out, nullptr, x, nullptr, nullptr, noise, nullptr, coef, nullptr, t_idx, N, voxels, 0, flags,
                       0, eta, sample, pred_xstart, stream});
}

int ddpm3d_dpm_solver_step(const float* model_out, const float* x, const float* x0_prev1, const float* x0_prev2,
                           const float* noise, const float* coef, const float* scoef, const int64_t* t_idx, int N,
                           int voxels, int T, int flags, int order, float* sample, float* pred_xstart, void* stream) {
    return step_entry("dpm_solver_step", STEP_SOLVER, STEP_PLAIN,
                      {model_out, nullptr, x, x0_prev1, x0_prev2, noise, nullptr, coef, scoef, t_idx, N, voxels, T, flags,
                       order, 0.0f, sample, pred_xstart, stream});
}

int ddpm3d_p_sample_step_keyed(const float* model_out, const float* x, const ddpm3d_noise_key* key, const float* coef,
                               const int64_t* t_idx, int N, int voxels, int flags, float* sample, float* pred_xstart,
                               void* stream) {
    return step_entry("p_sample_step_keyed", STEP_DDPM, STEP_KEYED,
                      {model_out, nullptr, x, nullptr, nullptr, nullptr, key, coef, nullptr, t_idx, N, voxels, 0, flags, 0,
                       0.0f, sample, pred_xstart, stream});
}

int ddpm3d_ddim_step_keyed(const float* model_out, const float* x, const ddpm3d_noise_key* key, const float* coef,
                           const int64_t* t_idx, int N, int voxels, int flags, float eta, float* sample,
                           float* pred_xstart, void* stream) {
    return step_entry("ddim_step_keyed", STEP_DDIM, STEP_KEYED,
                      {model_out, nullptr, x, nullptr, nullptr, nullptr, key, coef, nullptr, t_idx, N, voxels, 0, flags, 0,
                       eta, sample, pred_xstart, stream});
}

int ddpm3d_dpm_solver_step_keyed(const float* model_out, const float* x, const float* x0_prev1, const float* x0_prev2,
                                 const ddpm3d_noise_key* key, const float* coef, const float* scoef,
                                 const int64_t* t_idx, int N, int voxels, int T, int flags, int order, float* sample,
                                 float* pred_xstart, void* stream) {
    return step_entry("dpm_solver_step_keyed", STEP_SOLVER, STEP_KEYED,
                      {model_out, nullptr, x, x0_prev1, x0_prev2, nullptr, key, coef, scoef, t_idx, N, voxels, T, flags,
                       order, 0.0f, sample, pred_xstart, stream});
}

int ddpm3d_p_sample_step_x0(const float* model_out, const float* xstart, const float* x, const float* noise,
                            const ddpm3d_noise_key* key, const float* coef, const int64_t* t_idx, int N, int voxels,
                            int flags, float* sample, float* pred_xstart, void* stream) {
    return step_entry("p_sample_step_x0", STEP_DDPM, STEP_X0,
                      {model_out, xstart, x, nullptr, nullptr, noise, key, coef, nullptr, t_idx, N, voxels, 0, flags, 0,
                       0.0f, sample, pred_xstart, stream});
}

int ddpm3d_ddim_step_x0(const float* model_out, const float* xstart, const float* x, const float* noise,
                        const ddpm3d_noise_key* key, const float* coef, const int64_t* t_idx, int N, int voxels,
                        int flags, float eta, float* sample, float* pred_xstart, void* stream) {
    return step_entry("ddim_step_x0", STEP_DDIM, STEP_X0,
                      {model_out, xstart, x, nullptr, nullptr, noise, key, coef, nullptr, t_idx, N, voxels, 0, flags, 0,
                       eta, sample, pred_xstart, stream});
}

int ddpm3d_dpm_solver_step_x0(const float* model_out, const float* xstart, const float* x, const float* x0_prev1,
                              const float* x0_prev2, const float* noise, const ddpm3d_noise_key* key,
                              const float* coef, const float* scoef, const int64_t* t_idx, int N, int voxels, int T,
                              int flags, int order, float* sample, float* pred_xstart, void* stream) {
    return step_entry("dpm_solver_step_x0", STEP_SOLVER, STEP_X0,
                      {model_out, xstart, x, x0_prev1, x0_prev2, noise, key, coef, scoef, t_idx, N, voxels, T, flags,
                       order, 0.0f, sample, pred_xstart, stream});
}

int ddpm3d_q_sample_keyed(const float* x_start, const ddpm3d_noise_key* key, const float* qcoef, const int64_t* t_idx,
                          int N, int voxels, int T, float* x_t, void* stream) {
    const int rc = noise_key_ok("q_sample_keyed", key, N, voxels, true);
    if (rc != DDPM3D_OK) return rc;
    if (!x_start || !qcoef || !t_idx || !x_t || T <= 0)
        return fail(DDPM3D_EINVAL, "q_sample_keyed: bad arguments (N=%d voxels=%d T=%d)", N, voxels, T);
    return launched(ddpm3d_launch_q_sample(x_start, nullptr, key, qcoef, t_idx, N, voxels, T, x_t,
                                           (hipStream_t)stream),
                    "q_sample_keyed");
}

// ------------------------------------------------- uncertainty maps from K draws (added within ABI 13)
int ddpm3d_draw_stitch(const float* samples, int K, int res, const double* window, int xs, int ys, int zs, int H,
                       int W, int D, float* acc, float* wsum, void* stream) {
    if (!samples || !window || !acc || !wsum)
        return fail(DDPM3D_EINVAL, "draw_stitch: null pointer");
    if (K < 1 || K > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "draw_stitch: K=%d draws (1..%d)", K, DDPM3D_MAX_DRAWS);
    if (res < 1 || res > 1024 || H < 1 || W < 1 || D < 1)
        return fail(DDPM3D_EINVAL, "draw_stitch: bad shape (res=%d, volume H=%d W=%d D=%d)", res, H, W, D);
    if (xs < 0 || ys < 0 || zs < 0 || xs >= H || ys >= W || zs >= D)
        return fail(DDPM3D_EINVAL, "draw_stitch: patch origin (%d, %d, %d) outside the %dx%dx%d volume", xs, ys, zs,
                    H, W, D);
    return launched(ddpm3d_launch_draw_stitch(samples, K, res, window, xs, ys, zs, H, W, D, acc, wsum,
                                              (hipStream_t)stream),
                    "draw_stitch");
}

int ddpm3d_draw_moments(const float* acc, const float* wsum, int K, int64_t voxels, float* mean, float* std,
                        void* stream) {
    if (!acc || !mean || !std) return fail(DDPM3D_EINVAL, "draw_moments: null pointer");
    if (K < 2 || K > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "draw_moments: K=%d draws (2..%d)", K, DDPM3D_MAX_DRAWS);
    // one thread per voxel in the unaligned form: the grid's x extent bounds the volume
    if (voxels <= 0 || voxels > ((int64_t)0x7fffffff) * 256)
        return fail(DDPM3D_EINVAL, "draw_moments: voxels=%lld", (long long)voxels);
    return launched(ddpm3d_launch_draw_moments(acc, wsum, K, voxels, mean, std, (hipStream_t)stream),
                    "draw_moments");
}

int ddpm3d_draw_quantiles(const float* acc, const float* wsum, int K, int64_t voxels, int nq, const int* lower,
                          const float* frac, const float* target, float* quant, uint8_t* below, uint8_t* equal,
                          void* stream) {
    if (!acc) return fail(DDPM3D_EINVAL, "draw_quantiles: null pointer");
    if (K < 2 || K > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "draw_quantiles: K=%d draws (2..%d)", K, DDPM3D_MAX_DRAWS);
    // one thread per voxel: the grid's x extent bounds the volume
    if (voxels <= 0 || voxels > ((int64_t)0x7fffffff) * 256)
        return fail(DDPM3D_EINVAL, "draw_quantiles: voxels=%lld", (long long)voxels);
    if (nq < 0 || nq > DDPM3D_MAX_QUANTILES)
        return fail(DDPM3D_EINVAL, "draw_quantiles: nq=%d quantiles (0..%d)", nq, DDPM3D_MAX_QUANTILES);
    if ((target != nullptr) != (below != nullptr) || (target != nullptr) != (equal != nullptr))
        return fail(DDPM3D_EINVAL, "draw_quantiles: target, below and equal come together or not at all");
    if (nq == 0 && !target) return fail(DDPM3D_EINVAL, "draw_quantiles: no quantile and no target: nothing to do");
    if (nq > 0 && (!quant || !lower || !frac))
        return fail(DDPM3D_EINVAL, "draw_quantiles: null quant, lower or frac with nq=%d", nq);
    ddpm3d_quantile_pos pos = {};
    for (int i = 0; i < nq; ++i) {
        if (lower[i] < 0 || lower[i] > K - 1)
            return fail(DDPM3D_EINVAL, "draw_quantiles: lower[%d]=%d outside 0..%d", i, lower[i], K - 1);
        if (!(frac[i] >= 0.0f && frac[i] < 1.0f))
            return fail(DDPM3D_EINVAL, "draw_quantiles: frac[%d]=%g outside [0, 1)", i, (double)frac[i]);
        if (lower[i] == K - 1 && frac[i] != 0.0f)
            return fail(DDPM3D_EINVAL, "draw_quantiles: lower[%d]=%d is the last draw but frac=%g", i, lower[i],
                        (double)frac[i]);
        pos.lower[i] = lower[i];
        pos.frac[i] = frac[i];
    }
    return launched(ddpm3d_launch_draw_quantiles(acc, wsum, K, voxels, nq, pos, target, quant, below, equal,
                                                 (hipStream_t)stream),
                    "draw_quantiles");
}

// ------------------------------------------------- patch gather and blend: joint patch sampling and sliding-window
// tiling (both added within ABI 13) check their canvases and their starts, axis by axis, through the same two functions
static int canvas_check(const char* what, int B, int Dc, int H, int W, int res) {
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "%s: B=%d canvases (1..%d)", what, B, DDPM3D_MAX_DRAWS);
    if (res < 1 || res > 1024) return fail(DDPM3D_EINVAL, "%s: res=%d (1..1024)", what, res);
    // the grids put depth on y and the draws (times the patches) on z; one plane, rounded up to whole workgroups
    // of 256, is indexed in 32 bits
    if (Dc < 1 || H < 1 || W < 1 || Dc > 65535 || H > 65535 || W > 65535 || (int64_t)H * W > 0x7fffffff - 256)
        return fail(DDPM3D_EINVAL, "%s: bad canvas (Dc=%d H=%d W=%d; 1..65535 each, H * W <= 2^31 - 257)", what, Dc, H,
                    W);
    return DDPM3D_OK;
}

struct patch_axis { const char* name; int n; const int32_t* starts; int extent; };

// The host starts of each axis.  ascending: the tiles entries' rule (any number of strictly ascending starts);
// otherwise the joint entries' (at most DDPM3D_JOINT_MAX_STARTS, any order, repeats allowed).  cover: the union of
// [start, start + res) must hold every coordinate of the axis.
static int axes_check(const char* what, const patch_axis (&axes)[3], int res, bool ascending, bool cover) {
    for (const patch_axis& a : axes) {
        const int n = a.n, extent = a.extent;
        const int32_t* s = a.starts;
        if (ascending) {
            // a patch covers at least one coordinate of its own, so an axis holds at most `extent` ascending starts
            if (n < 1 || n > extent || !s)
                return fail(DDPM3D_EINVAL, "%s: %d starts on axis %s (1..%d, not NULL)", what, n, a.name, extent);
        } else if (n < 1 || n > DDPM3D_JOINT_MAX_STARTS) {
            return fail(DDPM3D_EINVAL, "%s: %d starts on axis %s (1..%d)", what, n, a.name, DDPM3D_JOINT_MAX_STARTS);
        }
        for (int i = 0; i < n; ++i) {
            if (s[i] < 0 || s[i] > extent - res)
                return fail(DDPM3D_EINVAL, "%s: patch at %d on axis %s outside the canvas (starts 0..%d)", what, s[i],
                            a.name, extent - res);
            if (ascending && i && s[i] <= s[i - 1])
                return fail(DDPM3D_EINVAL, "%s: starts on axis %s do not ascend (%d after %d)", what, a.name, s[i],
                            s[i - 1]);
        }
        if (!cover) continue;
        int gap = -1;                             // the first coordinate that no patch covers
        if (ascending) {
            // the union is the axis iff it begins at 0, ends at the extent and no neighbour starts beyond its
            // predecessor's end
            if (s[0] > 0) gap = 0;
            for (int i = 1; i < n && gap < 0; ++i)
                if (s[i] > s[i - 1] + res) gap = s[i - 1] + res;
            if (gap < 0 && s[n - 1] + res < extent) gap = s[n - 1] + res;
        } else {
            // any order: sweep from 0, always taking the start that reaches furthest among those at or below the
            // first uncovered coordinate
            for (int reach = 0; reach < extent && gap < 0;) {
                int next = reach;
                for (int i = 0; i < n; ++i)
                    if (s[i] <= reach && s[i] + res > next) next = s[i] + res;
                if (next == reach) gap = reach;
                reach = next;
            }
        }
        if (gap >= 0)
            return fail(DDPM3D_EINVAL, "%s: coordinate %d of axis %s is covered by no patch", what, gap, a.name);
    }
    return DDPM3D_OK;
}

static int joint_check(const char* what, int B, int Dc, int H, int W, int res, const ddpm3d_joint_starts* s,
                       bool covered) {
    const int rc = canvas_check(what, B, Dc, H, W, res);
    if (rc != DDPM3D_OK) return rc;
    const patch_axis axes[3] = {{"H", s->nx, s->xs, H}, {"W", s->ny, s->ys, W}, {"D", s->nz, s->zs, Dc}};
    return axes_check(what, axes, res, false, covered);
}

int ddpm3d_joint_gather(const float* canvas, int B, int Dc, int H, int W, int res, const ddpm3d_joint_starts* starts,
                        int first_patch, int n_patches, float* out, void* stream) {
    if (!canvas || !starts || !out) return fail(DDPM3D_EINVAL, "joint_gather: null pointer");
    const int rc = joint_check("joint_gather", B, Dc, H, W, res, starts, false);
    if (rc != DDPM3D_OK) return rc;
    const int P = starts->nx * starts->ny * starts->nz;
    if (first_patch < 0 || n_patches < 1 || first_patch > P - n_patches)
        return fail(DDPM3D_EINVAL, "joint_gather: patches %d..%d of %d", first_patch, first_patch + n_patches - 1, P);
    return launched(ddpm3d_launch_joint_gather(canvas, B, Dc, H, W, res, *starts, first_patch, n_patches, out,
                                               (hipStream_t)stream),
                    "joint_gather");
}

int ddpm3d_joint_blend(const float* patch_values, int B, int Dc, int H, int W, int res,
                       const ddpm3d_joint_starts* starts, const double* tables, float* out_canvas, void* stream) {
    if (!patch_values || !starts || !tables || !out_canvas) return fail(DDPM3D_EINVAL, "joint_blend: null pointer");
    const int rc = joint_check("joint_blend", B, Dc, H, W, res, starts, true);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_joint_blend(patch_values, B, Dc, H, W, res, *starts, tables, out_canvas,
                                              (hipStream_t)stream),
                    "joint_blend");
}

static int tiling_check(const char* what, int B, int Dc, int H, int W, int res, const ddpm3d_tiling* t, bool blend,
                        int64_t* patches) {
    int rc = canvas_check(what, B, Dc, H, W, res);
    if (rc != DDPM3D_OK) return rc;
    if (!t->d_starts || (blend && (!t->d_cover || !t->d_tables)))
        return fail(DDPM3D_EINVAL, "%s: null device table in the tiling descriptor", what);
    if (blend && ((reinterpret_cast<uintptr_t>(t->d_cover) | reinterpret_cast<uintptr_t>(t->d_tables)) & 7))
        return fail(DDPM3D_EINVAL, "%s: d_cover and d_tables must be 8-byte aligned", what);
    const patch_axis axes[3] = {{"H", t->n[0], t->starts[0], H}, {"W", t->n[1], t->starts[1], W},
                                {"D", t->n[2], t->starts[2], Dc}};
    rc = axes_check(what, axes, res, true, blend);
    if (rc != DDPM3D_OK) return rc;
    // rows are indexed in 32 bits inside the kernels, elements in 64; P is at most 65535^3 < 2^48
    const int64_t P = (int64_t)t->n[0] * t->n[1] * t->n[2];
    const int64_t rows = P * B, r3 = (int64_t)res * res * res;
    if (rows > 0x7fffffff || rows > ((int64_t)1 << 61) / r3)
        return fail(DDPM3D_EINVAL, "%s: %lld patches x %d canvases of %d^3 are too many rows", what, (long long)P, B,
                    res);
    *patches = P;
    return DDPM3D_OK;
}

int ddpm3d_tiles_gather(const float* canvas, int B, int Dc, int H, int W, int res, const ddpm3d_tiling* tiling,
                        int first_patch, int n_patches, float* out, void* stream) {
    if (!canvas || !tiling || !out) return fail(DDPM3D_EINVAL, "tiles_gather: null pointer");
    int64_t P = 0;
    const int rc = tiling_check("tiles_gather", B, Dc, H, W, res, tiling, false, &P);
    if (rc != DDPM3D_OK) return rc;
    if (first_patch < 0 || n_patches < 1 || first_patch > P - n_patches)
        return fail(DDPM3D_EINVAL, "tiles_gather: patches %d..%lld of %lld", first_patch,
                    (long long)first_patch + n_patches - 1, (long long)P);
    return launched(ddpm3d_launch_tiles_gather(canvas, B, Dc, H, W, res, *tiling, first_patch, n_patches, out,
                                               (hipStream_t)stream),
                    "tiles_gather");
}

int ddpm3d_tiles_blend(const float* patch_values, int B, int Dc, int H, int W, int res, const ddpm3d_tiling* tiling,
                       float* out_canvas, void* stream) {
    if (!patch_values || !tiling || !out_canvas) return fail(DDPM3D_EINVAL, "tiles_blend: null pointer");
    int64_t P = 0;
    const int rc = tiling_check("tiles_blend", B, Dc, H, W, res, tiling, true, &P);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_tiles_blend(patch_values, B, Dc, H, W, res, *tiling, out_canvas,
                                              (hipStream_t)stream),
                    "tiles_blend");
}

// ------------------------------------------------- image-quality metrics (added within ABI 13)
static const int64_t EM_MAX_VOXELS = (int64_t)1 << 40;
static bool ssim_shape_ok(int D, int H, int W) {
    return D >= 11 && H >= 11 && W >= 11 && D <= 65535 && H <= 65535 && W <= 65535 &&
           (int64_t)H * W <= 0x7fffffff && (int64_t)D * H * W <= EM_MAX_VOXELS;
}

size_t ddpm3d_error_moments_workspace_bytes(int B, int64_t voxels) {
    if (B < 1 || B > DDPM3D_MAX_DRAWS || voxels <= 0 || voxels > EM_MAX_VOXELS) return 0;
    return ddpm3d_em_workspace_bytes(B, voxels);
}

int ddpm3d_error_moments(const float* est, const float* target, const uint8_t* mask, const float* std, int B,
                         int64_t voxels, void* ws, size_t ws_bytes, double* out, void* stream) {
    if (!est || !target || !out) return fail(DDPM3D_EINVAL, "error_moments: null pointer");
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "error_moments: B=%d estimates (1..%d)", B, DDPM3D_MAX_DRAWS);
    if (voxels <= 0 || voxels > EM_MAX_VOXELS)
        return fail(DDPM3D_EINVAL, "error_moments: voxels=%lld (1..2^40)", (long long)voxels);
    const int rc = ws_ok("error_moments", ddpm3d_em_workspace_bytes(B, voxels), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_error_moments(est, target, mask, std, B, voxels, (double*)ws, out,
                                                (hipStream_t)stream),
                    "error_moments");
}

size_t ddpm3d_ssim3d_workspace_bytes(int B, int D, int H, int W) {
    if (B < 1 || B > DDPM3D_MAX_DRAWS || !ssim_shape_ok(D, H, W)) return 0;
    return ddpm3d_ss_workspace_bytes(B, D, H, W);
}

int ddpm3d_ssim3d(const float* est, const float* target, const uint8_t* mask, int B, int D, int H, int W, double C1,
                  double C2, void* ws, size_t ws_bytes, float* map, double* out, void* stream) {
    if (!est || !target || !out) return fail(DDPM3D_EINVAL, "ssim3d: null pointer");
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "ssim3d: B=%d estimates (1..%d)", B, DDPM3D_MAX_DRAWS);
    if (!ssim_shape_ok(D, H, W))
        return fail(DDPM3D_EINVAL, "ssim3d: bad volume (D=%d H=%d W=%d; 11..65535 each, H * W <= 2^31 - 1, "
                                   "D * H * W <= 2^40)", D, H, W);
    // !(c >= 0) also catches NaN; the kernel evaluates S in fp32, so the constants must be finite there
    if (!(C1 >= 0.0) || !(C2 >= 0.0) || C1 > 3.0e38 || C2 > 3.0e38)
        return fail(DDPM3D_EINVAL, "ssim3d: C1=%g C2=%g must be finite and not negative", C1, C2);
    const int rc = ws_ok("ssim3d", ddpm3d_ss_workspace_bytes(B, D, H, W), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_ssim3d(est, target, mask, B, D, H, W, (float)C1, (float)C2, (double*)ws, map, out,
                                         (hipStream_t)stream),
                    "ssim3d");
}

// ------------------------------------------------- per-step convergence trace (added within ABI 13)
static bool trace_shape_ok(int B, int64_t voxels) {
    return B >= 1 && B <= DDPM3D_TRACE_MAX_BATCH && voxels >= 1 && voxels <= EM_MAX_VOXELS;
}

size_t ddpm3d_trace_moments_workspace_bytes(int B, int64_t voxels) {
    if (!trace_shape_ok(B, voxels)) return 0;
    return ddpm3d_tr_workspace_bytes(B, voxels);
}

int ddpm3d_trace_moments(const float* est, const float* prev, const float* target, const float* weight, int B,
                         int64_t voxels, int64_t target_stride, int64_t weight_stride, void* ws, size_t ws_bytes,
                         double* out, void* stream) {
    if (!est || !out) return fail(DDPM3D_EINVAL, "trace_moments: null pointer");
    if (B < 1 || B > DDPM3D_TRACE_MAX_BATCH)
        return fail(DDPM3D_EINVAL, "trace_moments: B=%d estimates (1..%d)", B, DDPM3D_TRACE_MAX_BATCH);
    if (voxels <= 0 || voxels > EM_MAX_VOXELS)
        return fail(DDPM3D_EINVAL, "trace_moments: voxels=%lld (1..2^40)", (long long)voxels);
    if ((target_stride != 0 && target_stride != voxels) || (weight_stride != 0 && weight_stride != voxels))
        return fail(DDPM3D_EINVAL, "trace_moments: target_stride=%lld weight_stride=%lld (each 0, shared, or %lld)",
                    (long long)target_stride, (long long)weight_stride, (long long)voxels);
    if ((!target && target_stride != 0) || (!weight && weight_stride != 0))
        return fail(DDPM3D_EINVAL, "trace_moments: a NULL target / weight takes stride 0");
    const int rc = ws_ok("trace_moments", ddpm3d_tr_workspace_bytes(B, voxels), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_trace_moments(est, prev, target, weight, B, voxels, target_stride, weight_stride,
                                                (double*)ws, out, (hipStream_t)stream),
                    "trace_moments");
}

// ------------------------------------------------- multi-scale SSIM (added within ABI 13)
int ddpm3d_pool2(const float* vol, const uint8_t* mask, int B, int D, int H, int W, float* out, uint8_t* mask_out,
                 void* stream) {
    if (!vol || !out) return fail(DDPM3D_EINVAL, "pool2: null pointer");
    if ((mask == nullptr) != (mask_out == nullptr))
        return fail(DDPM3D_EINVAL, "pool2: mask and mask_out must both be given or both be NULL");
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "pool2: B=%d volumes (1..%d)", B, DDPM3D_MAX_DRAWS);
    if (D < 2 || H < 2 || W < 2 || D > 65535 || H > 65535 || W > 65535 || (int64_t)H * W > 0x7fffffff ||
        (int64_t)D * H * W > EM_MAX_VOXELS)
        return fail(DDPM3D_EINVAL, "pool2: bad volume (D=%d H=%d W=%d; 2..65535 each, H * W <= 2^31 - 1, "
                                   "D * H * W <= 2^40)", D, H, W);
    return launched(ddpm3d_launch_pool2(vol, mask, B, D, H, W, out, mask_out, (hipStream_t)stream), "pool2");
}

static bool msssim_shape_ok(int D, int H, int W, int scales) {
    if (scales < 1 || scales > DDPM3D_MSSSIM_MAX_SCALES || !ssim_shape_ok(D, H, W)) return false;
    return (D >> (scales - 1)) >= 11 && (H >> (scales - 1)) >= 11 && (W >> (scales - 1)) >= 11;
}

size_t ddpm3d_msssim3d_workspace_bytes(int B, int D, int H, int W, int scales) {
    if (B < 1 || B > DDPM3D_MAX_DRAWS || !msssim_shape_ok(D, H, W, scales)) return 0;
    return ddpm3d_ms_workspace_bytes(B, D, H, W, scales);
}

int ddpm3d_msssim3d(const float* est, const float* target, const uint8_t* mask, int B, int D, int H, int W, int scales,
                    double C1, double C2, void* ws, size_t ws_bytes, double* out, void* stream) {
    if (!est || !target || !out) return fail(DDPM3D_EINVAL, "msssim3d: null pointer");
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "msssim3d: B=%d estimates (1..%d)", B, DDPM3D_MAX_DRAWS);
    if (scales < 1 || scales > DDPM3D_MSSSIM_MAX_SCALES)
        return fail(DDPM3D_EINVAL, "msssim3d: scales=%d (1..%d)", scales, DDPM3D_MSSSIM_MAX_SCALES);
    if (!msssim_shape_ok(D, H, W, scales))
        return fail(DDPM3D_EINVAL, "msssim3d: bad volume for %d scales (D=%d H=%d W=%d; each at most 65535 and at "
                                   "least 11 after %d halvings, H * W <= 2^31 - 1, D * H * W <= 2^40)", scales, D, H, W,
                    scales - 1);
    // !(c >= 0) also catches NaN; the kernel evaluates S in fp32, so the constants must be finite there
    if (!(C1 >= 0.0) || !(C2 >= 0.0) || C1 > 3.0e38 || C2 > 3.0e38)
        return fail(DDPM3D_EINVAL, "msssim3d: C1=%g C2=%g must be finite and not negative", C1, C2);
    const int rc = ws_ok("msssim3d", ddpm3d_ms_workspace_bytes(B, D, H, W, scales), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_msssim3d(est, target, mask, B, D, H, W, scales, (float)C1, (float)C2, ws, out,
                                           (hipStream_t)stream),
                    "msssim3d");
}

// ------------------------------------------------- per-region moments (added within ABI 13)
// Checks the host side of a region index; *chunks receives the number of chunks all regions are cut into.
static int roi_index_check(const char* what, int B, const ddpm3d_roi_index* ix, int64_t* chunks) {
    if (!ix || !ix->offsets || !ix->d_offsets || !ix->d_chunks || !ix->d_index)
        return fail(DDPM3D_EINVAL, "%s: null pointer in the region index", what);
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "%s: B=%d estimates (1..%d)", what, B, DDPM3D_MAX_DRAWS);
    if (ix->regions < 1 || ix->regions > DDPM3D_ROI_MAX_REGIONS)
        return fail(DDPM3D_EINVAL, "%s: %d regions (1..%d)", what, ix->regions, DDPM3D_ROI_MAX_REGIONS);
    if (ix->entries < 0 || ix->entries > EM_MAX_VOXELS)
        return fail(DDPM3D_EINVAL, "%s: entries=%lld (0..2^40)", what, (long long)ix->entries);
    if (ix->offsets[0] != 0)
        return fail(DDPM3D_EINVAL, "%s: offsets[0]=%lld, not 0", what, (long long)ix->offsets[0]);
    int64_t n = 0;
    for (int r = 0; r < ix->regions; ++r) {
        const int64_t len = ix->offsets[r + 1] - ix->offsets[r];
        if (len < 0 || ix->offsets[r + 1] > ix->entries)
            return fail(DDPM3D_EINVAL, "%s: offsets[%d]=%lld after %lld (non-decreasing, at most entries=%lld)", what,
                        r + 1, (long long)ix->offsets[r + 1], (long long)ix->offsets[r], (long long)ix->entries);
        n += (len + DDPM3D_ROI_CHUNK - 1) / DDPM3D_ROI_CHUNK;
    }
    if (ix->offsets[ix->regions] != ix->entries)
        return fail(DDPM3D_EINVAL, "%s: offsets end at %lld, not at entries=%lld", what,
                    (long long)ix->offsets[ix->regions], (long long)ix->entries);
    *chunks = n;                                  // at most 2^40 / 4096 + 4096: a grid's x extent
    return DDPM3D_OK;
}
static size_t roi_ws_bytes(int B, int64_t chunks) {
    return (size_t)B * (size_t)(chunks > 0 ? chunks : 1) * DDPM3D_ROI_REC * sizeof(double);
}

size_t ddpm3d_roi_moments_workspace_bytes(int B, const ddpm3d_roi_index* index) {
    int64_t chunks = 0;
    return roi_index_check("roi_moments", B, index, &chunks) == DDPM3D_OK ? roi_ws_bytes(B, chunks) : 0;
}

int ddpm3d_roi_moments(const float* est, const float* target, int B, int64_t voxels, const ddpm3d_roi_index* index,
                       void* ws, size_t ws_bytes, double* out, void* stream) {
    if (!est || !out) return fail(DDPM3D_EINVAL, "roi_moments: null pointer");
    if (voxels <= 0 || voxels > EM_MAX_VOXELS)
        return fail(DDPM3D_EINVAL, "roi_moments: voxels=%lld (1..2^40)", (long long)voxels);
    int64_t chunks = 0;
    int rc = roi_index_check("roi_moments", B, index, &chunks);
    if (rc != DDPM3D_OK) return rc;
    rc = ws_ok("roi_moments", roi_ws_bytes(B, chunks), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_roi_moments(est, target, B, voxels, *index, chunks, (double*)ws, out,
                                              (hipStream_t)stream),
                    "roi_moments");
}

// ------------------------------------------------- per-region co-occurrence matrices (added within ABI 13)
int ddpm3d_roi_texture(const float* est, int B, int D, int H, int W, const ddpm3d_roi_index* index,
                       const int16_t* region_of, const float* lo, const float* inv_w, int levels, uint64_t* glcm,
                       uint64_t* hist, uint64_t* counts, void* stream) {
    if (!est || !region_of || !lo || !inv_w || !glcm || !hist || !counts)
        return fail(DDPM3D_EINVAL, "roi_texture: null pointer");
    if (D < 1 || H < 1 || W < 1 || D > 65535 || H > 65535 || W > 65535 || (int64_t)D * H * W > 0x7fffffff)
        return fail(DDPM3D_EINVAL, "roi_texture: bad volume (D=%d H=%d W=%d; 1..65535 each, D * H * W <= 2^31 - 1)",
                    D, H, W);
    if (levels < 2 || levels > DDPM3D_TEX_MAX_LEVELS)
        return fail(DDPM3D_EINVAL, "roi_texture: %d grey levels (2..%d)", levels, DDPM3D_TEX_MAX_LEVELS);
    int64_t chunks = 0;
    const int rc = roi_index_check("roi_texture", B, index, &chunks);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_roi_texture(est, B, D, H, W, *index, chunks, region_of, lo, inv_w, levels, glcm,
                                              hist, counts, (hipStream_t)stream),
                    "roi_texture");
}

// ------------------------------------------------- radial spectra and shell correlation (added within ABI 13)
static bool spec_shape_ok(int B, int D, int H, int W) {
    const int lim = DDPM3D_SPEC_MAX_EXTENT;
    return B >= 1 && B <= DDPM3D_MAX_DRAWS && D >= 2 && H >= 2 && W >= 2 && D <= lim && H <= lim && W <= lim;
}
static int spec_shape_check(const char* what, int B, int D, int H, int W) {
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "%s: B=%d volumes (1..%d)", what, B, DDPM3D_MAX_DRAWS);
    if (!spec_shape_ok(B, D, H, W))
        return fail(DDPM3D_EINVAL, "%s: bad volume (D=%d H=%d W=%d; 2..%d each)", what, D, H, W,
                    DDPM3D_SPEC_MAX_EXTENT);
    return DDPM3D_OK;
}
static int spec_axes_check(const char* what, const ddpm3d_dft_axis* axes, int D, int H, int W) {
    if (!axes) return fail(DDPM3D_EINVAL, "%s: null pointer", what);
    const int n[3] = {D, H, W}, rows[3] = {D, H, W / 2 + 1};
    for (int a = 0; a < 3; ++a) {
        if (!axes[a].cos_t || !axes[a].sin_t) return fail(DDPM3D_EINVAL, "%s: null table in axes[%d]", what, a);
        if (axes[a].n != n[a] || axes[a].rows != rows[a])
            return fail(DDPM3D_EINVAL, "%s: axes[%d] is %d rows of n=%d, the shape wants %d rows of n=%d", what, a,
                        axes[a].rows, axes[a].n, rows[a], n[a]);
    }
    return DDPM3D_OK;
}

size_t ddpm3d_dft3_workspace_bytes(int B, int D, int H, int W) {
    return spec_shape_ok(B, D, H, W) ? ddpm3d_dft_workspace_bytes(B, D, H, W) : 0;
}

static int dft3_entry(const char* what, const float* vol, const float* pivot, int B, int D, int H, int W,
                      const ddpm3d_dft_axis* axes, void* ws, size_t ws_bytes, float* re, float* im, int only,
                      void* stream) {
    if (!vol || !re || !im) return fail(DDPM3D_EINVAL, "%s: null pointer", what);
    int rc = spec_shape_check(what, B, D, H, W);
    if (rc != DDPM3D_OK) return rc;
    rc = spec_axes_check(what, axes, D, H, W);
    if (rc != DDPM3D_OK) return rc;
    rc = ws_ok(what, ddpm3d_dft_workspace_bytes(B, D, H, W), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_dft3(vol, pivot, B, D, H, W, axes, ws, re, im, only, (hipStream_t)stream), what);
}

int ddpm3d_dft3(const float* vol, const float* pivot, int B, int D, int H, int W, const ddpm3d_dft_axis axes[3],
                void* ws, size_t ws_bytes, float* re, float* im, void* stream) {
    return dft3_entry("dft3", vol, pivot, B, D, H, W, axes, ws, ws_bytes, re, im, -1, stream);
}

int ddpm3d_dft3_pass(int pass, const float* vol, const float* pivot, int B, int D, int H, int W,
                     const ddpm3d_dft_axis axes[3], void* ws, size_t ws_bytes, float* re, float* im, void* stream) {
    if (pass < 0 || pass > 2) return fail(DDPM3D_EINVAL, "dft3_pass: pass %d (0 = W, 1 = H, 2 = D)", pass);
    return dft3_entry("dft3_pass", vol, pivot, B, D, H, W, axes, ws, ws_bytes, re, im, pass, stream);
}

size_t ddpm3d_shell_sums_workspace_bytes(int B, const ddpm3d_roi_index* shells) {
    int64_t chunks = 0;
    return roi_index_check("shell_sums", B, shells, &chunks) == DDPM3D_OK ? ddpm3d_sp_workspace_bytes(B, chunks) : 0;
}

int ddpm3d_shell_sums(const float* xre, const float* xim, const float* yre, const float* yim, int B, int D, int H,
                      int W, const ddpm3d_roi_index* shells, void* ws, size_t ws_bytes, double* out, void* stream) {
    if (!xre || !xim || !out) return fail(DDPM3D_EINVAL, "shell_sums: null pointer");
    if ((yre == nullptr) != (yim == nullptr))
        return fail(DDPM3D_EINVAL, "shell_sums: yre and yim must both be given or both be NULL");
    int rc = spec_shape_check("shell_sums", B, D, H, W);
    if (rc != DDPM3D_OK) return rc;
    int64_t chunks = 0;
    rc = roi_index_check("shell_sums", B, shells, &chunks);
    if (rc != DDPM3D_OK) return rc;
    rc = ws_ok("shell_sums", ddpm3d_sp_workspace_bytes(B, chunks), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_shell_sums(xre, xim, yre, yim, B, D, H, W, *shells, chunks, (double*)ws, out,
                                             (hipStream_t)stream),
                    "shell_sums");
}

size_t ddpm3d_shell_spectrum_workspace_bytes(int B, int D, int H, int W, const ddpm3d_roi_index* shells,
                                             int with_target) {
    int64_t chunks = 0;
    if (!spec_shape_ok(B, D, H, W) || roi_index_check("shell_spectrum", B, shells, &chunks) != DDPM3D_OK ||
        shells->entries != (int64_t)D * H * (W / 2 + 1))
        return 0;
    return ddpm3d_spectrum_workspace_bytes(B, D, H, W, chunks, with_target != 0);
}

int ddpm3d_shell_spectrum(const float* est, const float* est_pivot, const float* target, const float* target_pivot,
                          int B, int D, int H, int W, const ddpm3d_dft_axis axes[3], const ddpm3d_roi_index* shells,
                          void* ws, size_t ws_bytes, double* out, void* stream) {
    if (!est || !out) return fail(DDPM3D_EINVAL, "shell_spectrum: null pointer");
    int rc = spec_shape_check("shell_spectrum", B, D, H, W);
    if (rc != DDPM3D_OK) return rc;
    rc = spec_axes_check("shell_spectrum", axes, D, H, W);
    if (rc != DDPM3D_OK) return rc;
    int64_t chunks = 0;
    rc = roi_index_check("shell_spectrum", B, shells, &chunks);
    if (rc != DDPM3D_OK) return rc;
    if (shells->entries != (int64_t)D * H * (W / 2 + 1))
        return fail(DDPM3D_EINVAL, "shell_spectrum: the shell index has %lld entries, the half spectrum %lld",
                    (long long)shells->entries, (long long)D * H * (W / 2 + 1));
    rc = ws_ok("shell_spectrum", ddpm3d_spectrum_workspace_bytes(B, D, H, W, chunks, target != nullptr), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_shell_spectrum(est, est_pivot, target, target ? target_pivot : nullptr, B, D, H, W,
                                                 axes, *shells, chunks, ws, out, (hipStream_t)stream),
                    "shell_spectrum");
}

// ------------------------------------------------- connected components (added within ABI 13)
// a volume the dense kernels index with 32-bit voxel and row numbers: 1 or more each, D * H and D * H * W <= 2^31 - 1
static bool volume_shape_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H <= 0x7fffffff && (int64_t)D * H * W <= 0x7fffffff;
}

// the connectivity and the shape of the graph passes over a voxel volume: components, basins, basin saddles
static int voxel_graph_ok(const char* what, int connectivity, int D, int H, int W) {
    if (connectivity != 6 && connectivity != 18 && connectivity != 26)
        return fail(DDPM3D_EINVAL, "%s: connectivity %d (6, 18 or 26)", what, connectivity);
    if (!volume_shape_ok(D, H, W))
        return fail(DDPM3D_EINVAL, "%s: bad volume (D=%d H=%d W=%d; 1 or more each, D * H * W <= 2^31 - 1)", what, D,
                    H, W);
    return DDPM3D_OK;
}

size_t ddpm3d_label_components_workspace_bytes(int D, int H, int W) {
    return volume_shape_ok(D, H, W) ? ddpm3d_ccl_workspace_bytes(D, H, W) : 0;
}

int ddpm3d_label_components(const float* vol, const uint8_t* keep, float threshold, int connectivity, int D, int H,
                            int W, int32_t* roots, void* ws, size_t ws_bytes, int32_t* status, void* stream) {
    if (!vol || !roots || !status) return fail(DDPM3D_EINVAL, "label_components: null pointer");
    int rc = voxel_graph_ok("label_components", connectivity, D, H, W);
    if (rc != DDPM3D_OK) return rc;
    if (threshold != threshold) return fail(DDPM3D_EINVAL, "label_components: the threshold is NaN");
    rc = ws_ok("label_components", ddpm3d_ccl_workspace_bytes(D, H, W), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_label_components(vol, keep, threshold, connectivity, D, H, W, roots, ws, status,
                                                   (hipStream_t)stream),
                    "label_components");
}

// ------------------------------------------------- sphere-mean map for SUVpeak (added within ABI 13)
int ddpm3d_sphere_mean(const float* vol, const uint8_t* keep, int B, int D, int H, int W, int r0, int r1,
                       const int32_t* half_w, float* out, void* stream) {
    const int R = DDPM3D_PEAK_MAX_RADIUS;
    if (!vol || !out || !half_w) return fail(DDPM3D_EINVAL, "sphere_mean: null pointer");
    if (vol == out) return fail(DDPM3D_EINVAL, "sphere_mean: out must not be vol (every voxel is read by its neighbours)");
    if (B < 1 || B > DDPM3D_MAX_DRAWS)
        return fail(DDPM3D_EINVAL, "sphere_mean: B=%d volumes (1..%d)", B, DDPM3D_MAX_DRAWS);
    if (!volume_shape_ok(D, H, W))
        return fail(DDPM3D_EINVAL, "sphere_mean: bad volume (D=%d H=%d W=%d; 1 or more each, D * H * W <= 2^31 - 1)",
                    D, H, W);
    if (r0 < 0 || r0 > R || r1 < 0 || r1 > R)
        return fail(DDPM3D_EINVAL, "sphere_mean: radii r0=%d r1=%d (0..%d)", r0, r1, R);
    const int n0 = 2 * r0 + 1, n1 = 2 * r1 + 1;
    for (int i = 0; i < n0 * n1; ++i)
        if (half_w[i] < -1 || half_w[i] > R)
            return fail(DDPM3D_EINVAL, "sphere_mean: half_w[%d][%d]=%d (-1..%d)", i / n1, i % n1, half_w[i], R);
    if (half_w[r0 * n1 + r1] < 0) return fail(DDPM3D_EINVAL, "sphere_mean: the centre row half_w[%d][%d] is absent", r0, r1);
    for (int i = 0; i < n0; ++i)
        for (int j = 0; j < n1; ++j)
            if (half_w[i * n1 + j] != half_w[(n0 - 1 - i) * n1 + j] || half_w[i * n1 + j] != half_w[i * n1 + n1 - 1 - j])
                return fail(DDPM3D_EINVAL, "sphere_mean: half_w is not symmetric under dz -> -dz and dy -> -dy (at [%d][%d])",
                            i, j);
    return launched(ddpm3d_launch_sphere_mean(vol, keep, B, D, H, W, r0, r1, half_w, out, (hipStream_t)stream),
                    "sphere_mean");
}

// ------------------------------------------------- baseline denoisers (added within ABI 13)
size_t ddpm3d_gauss_smooth_workspace_bytes(int D, int H, int W) {
    return volume_shape_ok(D, H, W) ? (((size_t)D * H * W * sizeof(float) + 15) & ~(size_t)15) : 0;
}

// the radii (0..DDPM3D_SMOOTH_MAX_RADIUS) and the host tap tables (positive, finite, symmetric) of a Gaussian entry
static int smooth_taps_ok(const char* what, const int radii[3], const float* const taps[3]) {
    const int R = DDPM3D_SMOOTH_MAX_RADIUS;
    for (int a = 0; a < 3; ++a) {
        if (radii[a] < 0 || radii[a] > R)
            return fail(DDPM3D_EINVAL, "%s: radii r0=%d r1=%d r2=%d (0..%d)", what, radii[0], radii[1], radii[2], R);
        const int n = 2 * radii[a] + 1;
        for (int j = 0; j < n; ++j) {
            const float t = taps[a][j];
            if (!(t > 0.0f) || t > 3.402823466e38f)
                return fail(DDPM3D_EINVAL, "%s: taps%d[%d]=%g (positive and finite)", what, a, j, (double)t);
            if (t != taps[a][n - 1 - j])
                return fail(DDPM3D_EINVAL, "%s: taps%d is not symmetric (at [%d])", what, a, j);
        }
    }
    return DDPM3D_OK;
}

int ddpm3d_gauss_smooth(const float* vol, int D, int H, int W, int r0, int r1, int r2, const float* taps0,
                        const float* taps1, const float* taps2, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!vol || !out || !taps0 || !taps1 || !taps2) return fail(DDPM3D_EINVAL, "gauss_smooth: null pointer");
    if (vol == out) return fail(DDPM3D_EINVAL, "gauss_smooth: out must not be vol (every voxel is read by its neighbours)");
    if (!volume_shape_ok(D, H, W))
        return fail(DDPM3D_EINVAL, "gauss_smooth: bad volume (D=%d H=%d W=%d; 1 or more each, D * H * W <= 2^31 - 1)",
                    D, H, W);
    const int radii[3] = {r0, r1, r2};
    const float* taps[3] = {taps0, taps1, taps2};
    int rc = smooth_taps_ok("gauss_smooth", radii, taps);
    if (rc == DDPM3D_OK) rc = ws_ok("gauss_smooth", ddpm3d_gauss_smooth_workspace_bytes(D, H, W), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    if (ws == (const void*)vol || ws == (void*)out)
        return fail(DDPM3D_EINVAL, "gauss_smooth: the workspace must be neither vol nor out");
    return launched(ddpm3d_launch_gauss_smooth(vol, D, H, W, radii, taps, out, (float*)ws, (hipStream_t)stream),
                    "gauss_smooth");
}

int ddpm3d_nlm(const float* vol, int D, int H, int W, int s0, int s1, int s2, int p0, int p1, int p2, float h,
               float sigma, float* out, void* stream) {
    const int S = DDPM3D_NLM_MAX_SEARCH, P = DDPM3D_NLM_MAX_PATCH;
    if (!vol || !out) return fail(DDPM3D_EINVAL, "nlm: null pointer");
    if (vol == out) return fail(DDPM3D_EINVAL, "nlm: out must not be vol (every voxel is read by its neighbours)");
    if (!volume_shape_ok(D, H, W))
        return fail(DDPM3D_EINVAL, "nlm: bad volume (D=%d H=%d W=%d; 1 or more each, D * H * W <= 2^31 - 1)", D, H, W);
    if (s0 < 0 || s0 > S || s1 < 0 || s1 > S || s2 < 0 || s2 > S)
        return fail(DDPM3D_EINVAL, "nlm: search radii s0=%d s1=%d s2=%d (0..%d)", s0, s1, s2, S);
    if (p0 < 0 || p0 > P || p1 < 0 || p1 > P || p2 < 0 || p2 > P)
        return fail(DDPM3D_EINVAL, "nlm: patch radii p0=%d p1=%d p2=%d (0..%d)", p0, p1, p2, P);
    if (!(h > 0.0f) || h > 3.402823466e38f) return fail(DDPM3D_EINVAL, "nlm: h=%g (positive and finite)", (double)h);
    if (!(sigma >= 0.0f) || sigma > 3.402823466e38f)
        return fail(DDPM3D_EINVAL, "nlm: sigma=%g (0 or more, finite)", (double)sigma);
    // the two constants of the exponent, formed in fp64 and rounded once each
    const double n_p = (double)(2 * p0 + 1) * (2 * p1 + 1) * (2 * p2 + 1);
    const double k1 = 1.0 / (n_p * (double)h * (double)h), k2 = 2.0 * (double)sigma * (double)sigma / ((double)h * (double)h);
    if (k1 > 3.402823466e38 || k2 > 3.402823466e38)
        return fail(DDPM3D_EINVAL, "nlm: h=%g is too small: 1 / (n_p h^2) = %g and 2 sigma^2 / h^2 = %g must be finite "
                                   "in fp32", (double)h, k1, k2);
    const int search[3] = {s0, s1, s2}, patch[3] = {p0, p1, p2};
    return launched(ddpm3d_launch_nlm(vol, D, H, W, search, patch, (float)k1, (float)k2, out, (hipStream_t)stream), "nlm");
}

// ------------------------------------------------- volume regridding (added within ABI 13)
static const int64_t REGRID_MAX_VOXELS = 0x7fffffff;
// every stage of the chain, per volume: the input, the two intermediates and the output
static bool regrid_shape_ok(int D, int H, int W, int Do, int Ho, int Wo, int64_t stage[3]) {
    if (D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1) return false;
    if ((int64_t)D * H > REGRID_MAX_VOXELS || (int64_t)D * H * W > REGRID_MAX_VOXELS) return false;
    if ((int64_t)Do * Ho > REGRID_MAX_VOXELS || (int64_t)Ho * Wo > REGRID_MAX_VOXELS) return false;
    if ((int64_t)D * Ho > REGRID_MAX_VOXELS) return false;
    ddpm3d_regrid_stages(D, H, W, Do, Ho, Wo, stage);
    return stage[0] <= REGRID_MAX_VOXELS && stage[1] <= REGRID_MAX_VOXELS && stage[2] <= REGRID_MAX_VOXELS;
}
static bool regrid_ratio_ok(int in_len, int out_len) {
    return (int64_t)in_len <= 4 * (int64_t)out_len && (int64_t)out_len <= 4 * (int64_t)in_len;
}
static size_t regrid_ws_bytes(int B, const int64_t stage[3]) {
    const size_t a = ((size_t)B * stage[0] * sizeof(float) + 15) & ~(size_t)15;
    const size_t b = ((size_t)B * stage[1] * sizeof(float) + 15) & ~(size_t)15;
    return a + b;
}
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

size_t ddpm3d_regrid_workspace_bytes(int B, int D, int H, int W, int Do, int Ho, int Wo) {
    int64_t stage[3];
    if (B < 1 || B > DDPM3D_MAX_DRAWS || !regrid_shape_ok(D, H, W, Do, Ho, Wo, stage)) return 0;
    if (!regrid_ratio_ok(D, Do) || !regrid_ratio_ok(H, Ho) || !regrid_ratio_ok(W, Wo)) return 0;
    return regrid_ws_bytes(B, stage);
}

int ddpm3d_regrid(const float* vol, int B, int D, int H, int W, const ddpm3d_regrid_axis axes[3], float* out, void* ws,
                  size_t ws_bytes, void* stream) {
    if (!vol || !out || !axes) return fail(DDPM3D_EINVAL, "regrid: null pointer (vol, out or axes)");
    if (B < 1 || B > DDPM3D_MAX_DRAWS) return fail(DDPM3D_EINVAL, "regrid: B=%d volumes (1..%d)", B, DDPM3D_MAX_DRAWS);
    const int in_len[3] = {D, H, W};
    static const char* const name[3] = {"D", "H", "W"};
    for (int a = 0; a < 3; ++a) {
        const ddpm3d_regrid_axis& x = axes[a];
        if (x.taps < 0 || x.taps > DDPM3D_REGRID_MAX_TAPS)
            return fail(DDPM3D_EINVAL, "regrid: axes[%d] (%s): taps=%d (0..%d)", a, name[a], x.taps,
                        DDPM3D_REGRID_MAX_TAPS);
        if (x.in_len < 1 || x.out_len < 1)
            return fail(DDPM3D_EINVAL, "regrid: axes[%d] (%s): in_len=%d out_len=%d (1 or more each)", a, name[a],
                        x.in_len, x.out_len);
        if (x.in_len != in_len[a])
            return fail(DDPM3D_EINVAL, "regrid: axes[%d] (%s): in_len=%d, the volume has %s=%d", a, name[a], x.in_len,
                        name[a], in_len[a]);
        if (x.taps == 0 && x.in_len != x.out_len)
            return fail(DDPM3D_EINVAL, "regrid: axes[%d] (%s): taps=0 is the identity, but in_len=%d and out_len=%d "
                                       "differ", a, name[a], x.in_len, x.out_len);
        if (!regrid_ratio_ok(x.in_len, x.out_len))
            return fail(DDPM3D_EINVAL, "regrid: axes[%d] (%s): ratio in_len / out_len = %d / %d outside [1/4, 4]", a,
                        name[a], x.in_len, x.out_len);
        if (x.taps > 0 && (!x.first || !x.count || !x.weights))
            return fail(DDPM3D_EINVAL, "regrid: axes[%d] (%s): null pointer (first, count or weights)", a, name[a]);
    }
    const int Do = axes[0].out_len, Ho = axes[1].out_len, Wo = axes[2].out_len;
    int64_t stage[3];
    if (!regrid_shape_ok(D, H, W, Do, Ho, Wo, stage))
        return fail(DDPM3D_EINVAL, "regrid: bad shape (D=%d H=%d W=%d -> %d %d %d; 1 or more each and at most 2^31 - 1 "
                                   "voxels per volume before and after every pass)", D, H, W, Do, Ho, Wo);
    const int rc = ws_ok("regrid", regrid_ws_bytes(B, stage), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    const size_t vol_bytes = (size_t)B * D * H * W * sizeof(float), out_bytes = (size_t)B * stage[2] * sizeof(float);
    if (ranges_overlap(vol, vol_bytes, out, out_bytes))
        return fail(DDPM3D_EINVAL, "regrid: out overlaps vol (every voxel is read by its neighbours)");
    if (ranges_overlap(ws, regrid_ws_bytes(B, stage), vol, vol_bytes) ||
        ranges_overlap(ws, regrid_ws_bytes(B, stage), out, out_bytes))
        return fail(DDPM3D_EINVAL, "regrid: the workspace overlaps vol or out");
    return launched(ddpm3d_launch_regrid(vol, B, D, H, W, axes, out, (float*)ws, (hipStream_t)stream), "regrid");
}

// ------------------------------------------------- maximum-intensity and ray-sum projections (added within ABI 13)
static bool project_counts_ok(int angles, int bins, int samples) {
    return angles >= 1 && angles <= DDPM3D_PROJECT_MAX_ANGLES && bins >= 1 && bins <= DDPM3D_PROJECT_MAX_BINS &&
           samples >= 1 && samples <= DDPM3D_PROJECT_MAX_BINS;
}
static int project_counts_check(const char* what, int angles, int bins, int samples) {
    if (!project_counts_ok(angles, bins, samples))
        return fail(DDPM3D_EINVAL, "%s: angles=%d (1..%d), bins=%d and samples=%d (1..%d each)", what, angles,
                    DDPM3D_PROJECT_MAX_ANGLES, bins, samples, DDPM3D_PROJECT_MAX_BINS);
    return DDPM3D_OK;
}
static bool finite_f32(float v) { return v - v == 0.0f; }
static bool positive_finite(double v) { return v > 0.0 && v - v == 0.0; }

int ddpm3d_project_table_fill(int H, int W, double s1, double s2, double pitch, int bins, double step, int samples,
                              const double* angles_deg, int angles, ddpm3d_project_table* table) {
    if (!angles_deg || !table) return fail(DDPM3D_EINVAL, "project_table_fill: null pointer");
    if (H < 1 || W < 1) return fail(DDPM3D_EINVAL, "project_table_fill: bad slice (H=%d W=%d; 1 or more each)", H, W);
    if (!positive_finite(s1) || !positive_finite(s2) || !positive_finite(pitch) || !positive_finite(step))
        return fail(DDPM3D_EINVAL, "project_table_fill: spacing (%g, %g), pitch %g, step %g (positive and finite, mm)",
                    s1, s2, pitch, step);
    const int rc = project_counts_check("project_table_fill", angles, bins, samples);
    if (rc != DDPM3D_OK) return rc;
    ddpm3d_project_table t;
    memset(&t, 0, sizeof t);
    t.angles = angles, t.bins = bins, t.samples = samples, t.step = (float)step;
    const double mid_u = 0.5 * (bins - 1), mid_j = 0.5 * (samples - 1);
    for (int k = 0; k < angles; ++k) {
        const double deg = angles_deg[k];
        if (deg - deg != 0.0) return fail(DDPM3D_EINVAL, "project_table_fill: angles_deg[%d]=%g is not finite", k, deg);
        // exactly 0 or +-1 at multiples of 90 degrees
        const double turn = fmod(deg, 360.0), quarter = turn / 90.0;
        double c, s;
        if (quarter == floor(quarter)) {
            static const double qc[4] = {1.0, 0.0, -1.0, 0.0}, qs[4] = {0.0, 1.0, 0.0, -1.0};
            const int q = ((int)quarter % 4 + 4) % 4;
            c = qc[q], s = qs[q];
        } else {
            const double rad = turn * (3.14159265358979323846 / 180.0);
            c = cos(rad), s = sin(rad);
        }
        // h' = (a s + r c) / s1 + (H - 1) / 2 and w' = (a c - r s) / s2 + (W - 1) / 2 with a = (u - mid_u) pitch and
        // r = (j - mid_j) step, as origin + u * (per-u increment) + j * (per-j increment)
        const double hu = pitch * s / s1, hj = step * c / s1, wu = pitch * c / s2, wj = -step * s / s2;
        const double v[6] = {0.5 * (H - 1) - mid_u * hu - mid_j * hj, hu, hj,
                             0.5 * (W - 1) - mid_u * wu - mid_j * wj, wu, wj};
        for (int i = 0; i < 6; ++i) {
            t.coef[k][i] = (float)v[i];
            if (!finite_f32(t.coef[k][i]))
                return fail(DDPM3D_EINVAL, "project_table_fill: entry %d of angle %d (%g degrees) is not finite in "
                                           "fp32", i, k, deg);
        }
    }
    if (!finite_f32(t.step)) return fail(DDPM3D_EINVAL, "project_table_fill: the step %g is not finite in fp32", step);
    *table = t;
    return DDPM3D_OK;
}

int ddpm3d_project(const float* vol, int B, int D, int H, int W, const ddpm3d_project_table* table, int mode,
                   float* out, void* stream) {
    if (!vol || !out || !table) return fail(DDPM3D_EINVAL, "project: null pointer");
    if (B < 1 || B > DDPM3D_MAX_DRAWS) return fail(DDPM3D_EINVAL, "project: B=%d volumes (1..%d)", B, DDPM3D_MAX_DRAWS);
    if (mode != DDPM3D_PROJECT_MAX && mode != DDPM3D_PROJECT_SUM)
        return fail(DDPM3D_EINVAL, "project: mode %d (DDPM3D_PROJECT_MAX = %d or DDPM3D_PROJECT_SUM = %d)", mode,
                    DDPM3D_PROJECT_MAX, DDPM3D_PROJECT_SUM);
    const int rc = project_counts_check("project", table->angles, table->bins, table->samples);
    if (rc != DDPM3D_OK) return rc;
    const int64_t lim = 0x7fffffff;
    // H - 1 and W - 1 must be fp32 numbers: the counting rule compares against them
    if (D < 1 || H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24) || (int64_t)H * W > lim ||
        (int64_t)D * H * W > lim || (int64_t)B * D * H * W > lim)
        return fail(DDPM3D_EINVAL, "project: bad volumes (B=%d D=%d H=%d W=%d; 1 or more each, H and W <= 2^24, "
                                   "B * D * H * W <= 2^31 - 1)", B, D, H, W);
    // B * angles * bins <= 2^30, D <= 2^31 - 1: no overflow
    const int64_t out_voxels = (int64_t)B * table->angles * table->bins * D;
    if (out_voxels > lim)
        return fail(DDPM3D_EINVAL, "project: %lld outputs (B * angles * D * bins <= 2^31 - 1)", (long long)out_voxels);
    if (!finite_f32(table->step)) return fail(DDPM3D_EINVAL, "project: the table's step is not finite");
    for (int k = 0; k < table->angles; ++k)
        for (int i = 0; i < 6; ++i)
            if (!finite_f32(table->coef[k][i]))
                return fail(DDPM3D_EINVAL, "project: entry %d of the table's angle %d is not finite", i, k);
    if (ranges_overlap(vol, (size_t)B * D * H * W * sizeof(float), out, (size_t)out_voxels * sizeof(float)))
        return fail(DDPM3D_EINVAL, "project: out overlaps vol");
    return launched(ddpm3d_launch_project(vol, B, D, H, W, *table, mode, out, (hipStream_t)stream), "project");
}

// ------------------------------------------------- squared Euclidean distance transform (added within ABI 13)
int ddpm3d_distance_sq(const uint8_t* mask, int K, int D, int H, int W, int invert, double s0, double s1, double s2,
                       float* out, void* stream) {
    if (!mask || !out) return fail(DDPM3D_EINVAL, "distance_sq: null pointer");
    if (K < 1 || D < 1 || H < 1 || W < 1)
        return fail(DDPM3D_EINVAL, "distance_sq: bad volumes (K=%d D=%d H=%d W=%d; 1 or more each)", K, D, H, W);
    const int lim = DDPM3D_EDT_MAX_EXTENT;
    if (D > lim || H > lim || W > lim)
        return fail(DDPM3D_EINVAL, "distance_sq: a %d x %d x %d volume (every extent is at most %d)", D, H, W, lim);
    const int64_t top = 0x7fffffff, voxels = (int64_t)D * H * W;
    if (voxels > top) return fail(DDPM3D_EINVAL, "distance_sq: %lld voxels per volume (at most 2^31 - 1)", (long long)voxels);
    const int64_t cols = DDPM3D_EDT_COLUMNS;
    if ((int64_t)K * D * H > top || (int64_t)K * D * ((W + cols - 1) / cols) > top ||
        (int64_t)K * (((int64_t)H * W + cols - 1) / cols) > top)
        return fail(DDPM3D_EINVAL, "distance_sq: K=%d volumes of %d x %d x %d are more workgroups than one launch "
                                   "takes", K, D, H, W);
    const double sd[3] = {s0, s1, s2};
    float sf[3];
    for (int a = 0; a < 3; ++a) {
        sf[a] = positive_finite(sd[a]) ? (float)sd[a] : 0.0f;
        if (!(sf[a] > 0.0f) || !finite_f32(sf[a]))
            return fail(DDPM3D_EINVAL, "distance_sq: spacing (%g, %g, %g) mm (positive and finite, also in fp32)", s0,
                        s1, s2);
    }
    if (invert != 0 && invert != 1) return fail(DDPM3D_EINVAL, "distance_sq: invert=%d (0 or 1)", invert);
    if (ranges_overlap(mask, (size_t)K * voxels, out, (size_t)K * voxels * sizeof(float)))
        return fail(DDPM3D_EINVAL, "distance_sq: out overlaps mask");
    return launched(ddpm3d_launch_distance_sq(mask, K, D, H, W, invert, sf, out, (hipStream_t)stream), "distance_sq");
}

// ------------------------------------------------- watershed basins and their saddle graph (added within ABI 13)
size_t ddpm3d_basins_workspace_bytes(int D, int H, int W) {
    return volume_shape_ok(D, H, W) ? ddpm3d_watershed_workspace_bytes() : 0;
}

int ddpm3d_basins(const float* height, const int32_t* labels, int connectivity, int D, int H, int W, int32_t* peaks,
                  void* ws, size_t ws_bytes, int32_t* status, void* stream) {
    if (!height || !labels || !peaks || !status) return fail(DDPM3D_EINVAL, "basins: null pointer");
    int rc = voxel_graph_ok("basins", connectivity, D, H, W);
    if (rc == DDPM3D_OK) rc = ws_ok("basins", ddpm3d_watershed_workspace_bytes(), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    const size_t bytes = (size_t)D * H * W * 4;
    if (ranges_overlap(peaks, bytes, height, bytes) || ranges_overlap(peaks, bytes, labels, bytes))
        return fail(DDPM3D_EINVAL, "basins: peaks overlaps an input (every voxel is read by its neighbours)");
    return launched(ddpm3d_launch_basins(height, labels, connectivity, D, H, W, peaks, ws, status,
                                         (hipStream_t)stream), "basins");
}

size_t ddpm3d_basin_saddles_workspace_bytes(int D, int H, int W) {
    return volume_shape_ok(D, H, W) ? ddpm3d_watershed_workspace_bytes() : 0;
}

int ddpm3d_basin_saddles(const float* height, const int32_t* labels, const int32_t* peaks, int connectivity, int D,
                         int H, int W, int cap, int32_t* pairs, float* saddle, void* ws, size_t ws_bytes,
                         int32_t* status, void* stream) {
    if (!height || !labels || !peaks || !status) return fail(DDPM3D_EINVAL, "basin_saddles: null pointer");
    if (cap < 0) return fail(DDPM3D_EINVAL, "basin_saddles: capacity %d (0 or more records)", cap);
    if (cap > 0 && (!pairs || !saddle)) return fail(DDPM3D_EINVAL, "basin_saddles: null record buffer");
    int rc = voxel_graph_ok("basin_saddles", connectivity, D, H, W);
    if (rc == DDPM3D_OK) rc = ws_ok("basin_saddles", ddpm3d_watershed_workspace_bytes(), ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    return launched(ddpm3d_launch_basin_saddles(height, labels, peaks, connectivity, D, H, W, cap, pairs, saddle, ws,
                                                status, (hipStream_t)stream), "basin_saddles");
}

// ------------------------------------------------- low-pass pull of x_start (added within ABI 13)
static bool pull_shape_ok(int N, int D, int H, int W) {
    return N >= 1 && N <= 65535 && volume_shape_ok(D, H, W) && (int64_t)N * D * H * W <= 0x7fffffff;
}

size_t ddpm3d_xstart_pull_workspace_bytes(int N, int D, int H, int W) {
    return pull_shape_ok(N, D, H, W) ? (((size_t)N * D * H * W * sizeof(float) + 15) & ~(size_t)15) : 0;
}

int ddpm3d_xstart_pull(const float* model_out, const float* x, const float* measurement, const float* coef,
                       const int64_t* t_idx, int N, int D, int H, int W, int T, int flags, float weight, int r0, int r1,
                       int r2, const float* taps0, const float* taps1, const float* taps2, float* xstart_out, void* ws,
                       size_t ws_bytes, void* stream) {
    if (!model_out || !x || !measurement || !coef || !t_idx || !xstart_out || !taps0 || !taps1 || !taps2)
        return fail(DDPM3D_EINVAL, "xstart_pull: null pointer");
    if (!pull_shape_ok(N, D, H, W) || T < 1)
        return fail(DDPM3D_EINVAL, "xstart_pull: bad shape (N=%d D=%d H=%d W=%d T=%d; 1 or more each, N <= 65535, "
                                   "N * D * H * W <= 2^31 - 1)", N, D, H, W, T);
    if (flags & ~STEP_FLAGS) return fail(DDPM3D_EINVAL, "xstart_pull: unknown flag bits %#x", flags);
    if (!(weight >= 0.0f && weight <= 1.0f))
        return fail(DDPM3D_EINVAL, "xstart_pull: weight %g outside [0, 1]", (double)weight);
    const int radii[3] = {r0, r1, r2};
    const float* taps[3] = {taps0, taps1, taps2};
    const size_t need = ddpm3d_xstart_pull_workspace_bytes(N, D, H, W);
    int rc = smooth_taps_ok("xstart_pull", radii, taps);
    if (rc == DDPM3D_OK) rc = ws_ok("xstart_pull", need, ws, ws_bytes);
    if (rc != DDPM3D_OK) return rc;
    const size_t bytes = (size_t)N * D * H * W * sizeof(float);
    const size_t mo_bytes = bytes * ((flags & DDPM3D_F_LEARN_SIGMA) ? 2 : 1);
    if (ranges_overlap(xstart_out, bytes, model_out, mo_bytes) || ranges_overlap(xstart_out, bytes, x, bytes) ||
        ranges_overlap(xstart_out, bytes, measurement, bytes))
        return fail(DDPM3D_EINVAL, "xstart_pull: xstart_out overlaps an input (every voxel is read by its neighbours)");
    if (ranges_overlap(ws, need, xstart_out, bytes) || ranges_overlap(ws, need, model_out, mo_bytes) ||
        ranges_overlap(ws, need, x, bytes) || ranges_overlap(ws, need, measurement, bytes))
        return fail(DDPM3D_EINVAL, "xstart_pull: the workspace overlaps a tensor of the call");
    return launched(ddpm3d_launch_xstart_pull(model_out, x, measurement, coef, t_idx, N, D, H, W, T, flags, weight,
                                              radii, taps, xstart_out, (float*)ws, (hipStream_t)stream),
                    "xstart_pull");
}

double ddpm3d_mfma_probe_flops_per_iter(int kind) { return ddpm3d_probe_flops_per_iter(kind); }

int ddpm3d_mfma_probe(int kind, int iters, int blocks, float* out, uint64_t* clocks, void* stream) {
    if (!out || !clocks || iters <= 0 || blocks <= 0 || ddpm3d_probe_flops_per_iter(kind) == 0.0)
        return fail(DDPM3D_EINVAL, "mfma_probe: bad arguments (kind=%d iters=%d blocks=%d)", kind, iters, blocks);
    return launched(ddpm3d_launch_mfma_probe(kind, iters, blocks, out, (unsigned long long*)clocks,
                                             (hipStream_t)stream), "mfma_probe");
}

}  // extern "C"
