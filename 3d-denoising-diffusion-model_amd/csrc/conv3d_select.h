// Internal, host code only: which kernel instance a conv call runs.  ddpm3d_conv_select is the ONE place that decides it
// -- kernel, variant, tile form, tile counts, grid -- from the validated descriptor and the shape rule's ConvCfg; api.hip
// writes ConvK's tile counts from the record, the launchers only map it to the instantiation.
#pragma once
#include <stdio.h>
#include "conv3d_params.h"

#ifndef DDPM3D_WZ_T84
#define DDPM3D_WZ_T84 1     // measurement builds: 0 = 8x8x2 tiles wherever the plain / skip variants would take 8x4x4 ones
#endif
#ifndef SK_MIN_WGS
#define SK_MIN_WGS 512      // conv3d_skinny.hip: workgroups the depth segmentation keeps the grid above
#endif
#ifndef DDPM3D_PW_WIDE
#define DDPM3D_PW_WIDE 1    // conv1x1.hip: conv_epilogue's 16-byte store form (a template argument of its kernel)
#endif

enum { CONV_DIRECT = 0, CONV_WZ = 1, CONV_PW = 2, CONV_SKINNY = 3 };   // conv3d.hip, conv3d_wz.h, conv1x1.hip, conv3d_skinny.hip
enum { WZV_PLAIN = 0, WZV_UP = 1, WZV_SKIP = 2 };                      // conv3d_wz.h: the shipped form, PHASE, SKIP
struct ConvSel {
    int kernel;                   // CONV_*
    int arith;                    // direct, 1x1: the template's PREC (0, 1, 2, 5); Winograd-D, skinny: 0 f16x3, 1 f16, 2 bf16
                                  // (conv3d_stage.h's WZ_F16X3 / WZ_F16 / WZ_BF16)
    int variant, order;           // Winograd-D: WZV_*, and the issue order of a tap (template IL)
    int TX, TY, TZ;               // the tile form launched (skinny: an 8x8 column of TZ planes)
    int tilesX, tilesY, tilesZ;   // tiles of that form per sample = ConvK.tilesX/Y/Z
    int KS, WN, pipe;             // direct: taps per axis, waves along Cout (= MT), PIPEM
    int src16, nch;               // 1x1: src16 = 16-bit sources; skinny: 0 fp32, 1 bf16, 2 f16 sources, and nch = Cin / 16
    int hint;                     // ConvK.hint: the descriptor's, DDPM3D_HINT_UP_PHASE dropped where the phase form does not run
    size_t w_offset;              // bytes into w_packed of the image the kernel reads (the phase image sits behind the first)
    unsigned grid[3];
    // (the dynamic LDS size is a constant of the instantiation: each launch helper takes it from its kernel's geometry)
};

static inline int ddpm3d_src16(int io) { return !(io & DDPM3D_IO_SRC0_BF16) ? 0 : ((io & DDPM3D_IO_HALF_IS_F16) ? 2 : 1); }
// The Winograd-D tile form, 128 voxels each way: 4x4x8 (four z-pairs) below 8x8; 8x4x4 (two z-pairs; r03) where such
// tiles cover the volume with as many tiles as the 8x8x2 grid the shape rule counted, so that statistics rows and
// workspace are unchanged; else 8x8x2.  The plain and skip variants apply it to the output grid, the phase variant to
// the low-resolution one.
struct WzTile { int TX, TY, TZ; };
static inline WzTile ddpm3d_wz_tile(int D, int H, int W, bool t84) {
    if (!ddpm3d_tile8(H, W, 3)) return {4, 4, 8};
    if (t84 && H % 8 == 0 && D % 4 == 0) return {8, 4, 4};
    return {8, 8, 2};
}

// the 3x3x3 convs with one or two output channels that conv3d_skinny.hip instantiates: Cin = 32, 64, 128 (base widths);
// fp32 sources in the f16x3 / f16 arithmetic, bf16 sources in the bf16 mode and f16 sources in the f16 mode (the modes
// whose residual stream is 16-bit)
static inline bool ddpm3d_skinny_ok(const ddpm3d_conv_desc& d) {
    const int CinPad = ddpm3d_cin_pad(d.Cin), src16 = ddpm3d_src16(d.io_dtype);
    if (d.ksize != 3 || d.Cout > 2 || d.in_mode != DDPM3D_IN_SAME || d.C1 != 0 || d.stats || d.res_mode != DDPM3D_RES_NONE ||
        (CinPad != 32 && CinPad != 64 && CinPad != 128)) return false;
    if (d.precision == DDPM3D_PREC_BF16) return src16 == 1;
    if (d.precision == DDPM3D_PREC_F16) return src16 == 0 || src16 == 2;
    return d.precision == DDPM3D_PREC_F16X3 && src16 == 0;
}
// the 1x1x1 convs on raw inputs (ResBlock skip connections) that conv1x1.hip's register-fed GEMM takes (api.hip deals
// whole 32-channel blocks to the splits of a 1x1 conv, which is what that kernel walks)
// (r03 kept the split-f16 form above 1024 workgroups -- the three 256 -> 128 skip convs at 64^3 -- on conv3d.hip's
// kernel, 0.110 against 0.120 ms; with the lean epilogue (conv3d_epilogue.h, r04) a 1x1 workgroup is 7 k cycles
// shorter and the order is the other way round, 0.108 against 0.115: profiles/r04_lib_ab_conv1x1_cut_lean_epilogue.txt)
static inline bool ddpm3d_pw_ok(const ddpm3d_conv_desc& d, const ConvCfg& c) {
    const bool s0 = (d.io_dtype & DDPM3D_IO_SRC0_BF16) != 0, s1 = (d.io_dtype & DDPM3D_IO_SRC1_BF16) != 0;
    return d.ksize == 1 && (c.PREC == 1 || c.PREC == 2 || c.PREC == 5) && c.WN == 4 && c.MT == 4 &&
           d.in_mode == DDPM3D_IN_SAME && d.aff_a == nullptr && d.act == 0 && d.stats == nullptr &&
           d.Cout % 128 == 0 && d.Cin % 32 == 0 && d.C0 % 32 == 0 && (d.C1 == 0 || s0 == s1);
}

// d has passed conv_prepare's checks up to the hints; c is its shape rule (a forced split included).  skip_cx > 0: the
// call is ddpm3d_conv3d_skip's conv2 and the pair is one the fused form exists for, with skip_cx block-input channels.
static inline ConvSel ddpm3d_conv_select(const ddpm3d_conv_desc& d, const ConvCfg& c, int skip_cx) {
    ConvSel s = {};
    const int CoutPad = ddpm3d_cout_pad(d.Cout);
    s.hint = d.kernel_hint & ~DDPM3D_HINT_UP_PHASE;
    s.TX = s.TY = 1 << c.TXL;
    s.TZ = 128 / (s.TX * s.TY);
    s.KS = c.KS; s.WN = c.WN;
    s.src16 = ddpm3d_src16(d.io_dtype);
    int phases = 1;
    if (ddpm3d_skinny_ok(d)) {
        // 8x8 columns of TZ planes: depth segments as long as possible (less halo) while the grid fills the chip twice over
        s.kernel = CONV_SKINNY;
        s.arith = d.precision == DDPM3D_PREC_F16 ? 1 : (d.precision == DDPM3D_PREC_BF16 ? 2 : 0);
        s.nch = ddpm3d_cin_pad(d.Cin) / DDPM3D_CONV_CK;
        const long long cols = (long long)d.N * ((d.H + 7) / 8) * ((d.W + 7) / 8);
        s.TX = s.TY = 8; s.TZ = d.D;
        while (s.TZ > 4 && cols * ((d.D + s.TZ - 1) / s.TZ) < SK_MIN_WGS) s.TZ = (s.TZ + 1) / 2;
    } else if (ddpm3d_pw_ok(d, c)) {
        s.kernel = CONV_PW; s.arith = c.PREC;
    } else if (ddpm3d_prec_wz(d.precision)) {
        s.kernel = CONV_WZ;
        s.arith = d.precision == DDPM3D_PREC_F16_WZ ? 1 : (d.precision == DDPM3D_PREC_BF16_WZ ? 2 : 0);
        // kernel_hint bits 12..14 force an issue order (value = IL + 1) of the f16x3 form, which then keeps 8x8x2 tiles (A/B
        // measurements; identical arithmetic).  Built: 0, 1 (r02), 2, 4 (r03); 3, 5, 6 were measured and are not.  Else one
        // order: f16x3 IL 4 (weight loads first, reads behind, wave priority 1; r03_layer_ab_wz_issue_order.txt), f16 / bf16 0.
        const int forced = (d.kernel_hint & DDPM3D_HINT_WZ_ORDER_MASK) >> DDPM3D_HINT_WZ_ORDER_SHIFT;
        WzTile t = ddpm3d_wz_tile(d.D, d.H, d.W, DDPM3D_WZ_T84 && !forced);
        s.order = s.arith ? 0 : ((forced && t.TX == 8) ? forced - 1 : 4);
        if ((d.kernel_hint & DDPM3D_HINT_UP_PHASE) && d.precision == DDPM3D_PREC_F16X3_WZ && d.in_mode == DDPM3D_IN_UP &&
            !((d.H | d.W) & 1) && d.res_mode != DDPM3D_RES_POOL) {
            // an IN_UP conv as four 2x2 phase convs on the low-resolution source (conv3d_wz.h PHASE): taken only where
            // four phases x the low-resolution tiles are exactly the tiles the shape rule counted on the output grid --
            // statistics rows (one per workgroup), workspace and split then are what ddpm3d_conv_cfg reports
            const WzTile tl = ddpm3d_wz_tile(d.D, d.H / 2, d.W / 2, true);
            const long long low = (long long)((d.W / 2 + tl.TX - 1) / tl.TX) * ((d.H / 2 + tl.TY - 1) / tl.TY) *
                                  ((d.D + tl.TZ - 1) / tl.TZ);
            if (4 * low == (long long)c.tilesX * c.tilesY * c.tilesZ) {
                s.variant = WZV_UP; s.order = 4; t = tl; phases = 4;
                s.hint = d.kernel_hint;
                s.w_offset = ddpm3d_packed_image(d.Cout, d.Cin, 3, DDPM3D_PREC_F16X3_WZ).bytes();
            }
        }
        if (skip_cx > 0 && s.variant == WZV_PLAIN && ddpm3d_skip_fuse_rule(d.N, d.D, d.H, d.W, skip_cx, d.Cout, c))
            s.variant = WZV_SKIP;
        s.TX = t.TX; s.TY = t.TY; s.TZ = t.TZ;
    } else {
        s.kernel = CONV_DIRECT; s.arith = c.PREC;
        s.pipe = d.in_mode == DDPM3D_IN_STRIDE2 ? 2 : ((d.in_mode == DDPM3D_IN_SAME || d.in_mode == DDPM3D_IN_UP) ? 1 : 0);
    }
    const int Wg = phases == 4 ? d.W / 2 : d.W, Hg = phases == 4 ? d.H / 2 : d.H;
    s.tilesX = (Wg + s.TX - 1) / s.TX;
    s.tilesY = (Hg + s.TY - 1) / s.TY;
    s.tilesZ = (d.D + s.TZ - 1) / s.TZ;
    s.grid[0] = (unsigned)((long long)phases * d.N * s.tilesZ * s.tilesY * s.tilesX);
    s.grid[1] = s.kernel == CONV_SKINNY ? 1u : (unsigned)((CoutPad + 32 * s.WN - 1) / (32 * s.WN));
    s.grid[2] = s.kernel == CONV_SKINNY ? 1u : (unsigned)c.S;
    return s;
}
// conv3d_wz_kernel's MODE_ of a Winograd-D record (conv3d_stage.h: WZ_F16X3_UP = 3, WZ_F16X3_SKIP = 4)
static inline int ddpm3d_wz_mode(const ConvSel& s) { return s.variant == WZV_PLAIN ? s.arith : 2 + s.variant; }
// The record as the kernel template's name, every template argument an integer, defaults and bools included:
// what a kernel trace prints, less the return type, the namespace, the parameter list and the blanks.
static inline int ddpm3d_conv_sel_name(const ConvSel& s, char* name, size_t len) {
    const int txl = s.TX == 8 ? 3 : 2;
    switch (s.kernel) {
        case CONV_WZ:
            return snprintf(name, len, "conv3d_wz_kernel<%d,%d,%d,%d>", ddpm3d_wz_mode(s), s.order, s.TX, s.TY);
        case CONV_PW:
            return snprintf(name, len, "conv3d_pw_kernel<%d,%d,%d,%d,%d>", s.arith, s.src16 != 0, txl, txl, DDPM3D_PW_WIDE != 0);
        case CONV_SKINNY:
            return snprintf(name, len, "conv3d_skinny_kernel<%d,%d,%d>", s.arith, s.nch, s.src16);
    }
    return snprintf(name, len, "conv3d_kernel<%d,%d,%d,%d,%d,%d,%d>", s.arith, s.pipe, s.KS, s.WN, s.WN, txl, txl);
}

// the launchers: map a record to its instantiation; hipErrorInvalidValue for a record that has none
hipError_t ddpm3d_launch_conv(const ConvK& k, const ConvSel& s, hipStream_t st);            // conv3d.hip: any kernel
hipError_t ddpm3d_launch_conv_wz(const ConvK& k, const ConvSel& s, hipStream_t st);         // conv3d.hip (conv3d_p3.o)
hipError_t ddpm3d_launch_conv_skinny(const ConvK& k, const ConvSel& s, hipStream_t st);     // conv3d_skinny.hip
hipError_t ddpm3d_launch_conv_pw(const ConvK& k, const ConvSel& s, hipStream_t st);         // conv1x1.hip
hipError_t ddpm3d_launch_splitk_reduce(const ConvK& k, hipStream_t st);
