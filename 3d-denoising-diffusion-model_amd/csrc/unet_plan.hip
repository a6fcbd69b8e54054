// The whole-network level of the C ABI (include/ddpm3d.h, "whole network"): a UNet forward
// (unet.py:1015-1044, :1687-1694; ResBlock :236-256; AttentionBlock :296-305; Downsample / Upsample
// :102-105, :129-136) compiled ONCE per (model, N, D, H, W) into a flat list of this library's own per-op
// calls -- every buffer carved out of ONE caller-provided device arena -- and replayed by
// ddpm3d_unet_forward.  This is the only planner: the Python host (guided_diffusion/engine.py: _Plan) reads the
// list with ddpm3d_unet_plan_steps and issues the same calls itself, launch by launch -- same calls, same
// arguments, same order, hence bit-identical results (tests/test_gpu_plan_golden.py).  Host code only: no
// kernel lives here.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <new>
#include <vector>
#include "ddpm3d.h"

namespace {

struct Act {                 // an NDHWC activation of the plan, with the GroupNorm partial sums its producer writes
    size_t off = 0;          // byte offset in the arena
    int C = 0, D = 0, H = 0, W = 0;
    int esize = 4;           // bytes per element (2 = the 16-bit residual stream of the f16 / bf16 modes)
    size_t stats_off = 0;
    int rows = 0;
    size_t bytes(int N) const { return (size_t)N * D * H * W * C * esize; }
    long long voxels() const { return (long long)D * H * W; }
};

struct Step {                // one call of the list: its public record, and the descriptors a conv record points at
    ddpm3d_plan_step rec;
    ddpm3d_conv_desc conv;
    ddpm3d_conv_skip skip;
};

Step new_step(int kind) {
    Step st;
    memset(&st, 0, sizeof(st));
    st.rec.kind = kind;
    return st;
}

struct Planner {
    const ddpm3d_unet_desc& m;
    int N, D, H, W;
    char* base;                                   // arena (never dereferenced here)
    size_t end;                                   // its size, rounded down to 256 (while sizing: far away)
    size_t top = 0, tail = 0;                     // bytes used at the front / at the end
    std::map<std::pair<size_t, int>, std::vector<size_t>> pool;   // (bytes, esize) -> free activation buffers
    std::vector<Step> steps;
    std::vector<int> ws_steps;                    // conv steps that use the shared split-K workspace
    size_t ws_bytes = 0, ws_off = 0;
    size_t in_absmax = 0;
    int half_esize;                               // 2 in the f16 / bf16 modes
    bool scaled, f16;
    char err[256] = "";
    int code = DDPM3D_EINVAL;                     // what a failed build returns (DDPM3D_E2BIG: split the batch)

    Planner(const ddpm3d_unet_desc& d, int n, int dd, int hh, int ww, char* b, size_t arena_bytes)
        : m(d), N(n), D(dd), H(hh), W(ww), base(b), end(arena_bytes & ~(size_t)255) {
        half_esize = (m.arithmetic == DDPM3D_PREC_F16 || m.arithmetic == DDPM3D_PREC_BF16) ? 2 : 4;
        f16 = m.arithmetic == DDPM3D_PREC_F16;
        scaled = m.arithmetic == DDPM3D_PREC_F16X3 || m.arithmetic == DDPM3D_PREC_F16;
    }
    bool fail(const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
        return false;
    }
    // Two bump regions in one arena.  Activations and the split-K workspace grow from the front at page (4 KiB)
    // alignment: the conv kernels run measurably slower on activations that start inside a page (published network,
    // bf16, 1x64^3: 7.17 against 7.14 ms per forward) -- what one allocation per tensor gave
    // the Python planner for free.  Their sizes are multiples of a page at every level that matters, so this costs
    // no padding there.  The many small buffers (statistics rows, GroupNorm coefficients, bounds) are packed at 256
    // bytes from the end downwards, so that they never push an activation off its page boundary.
    size_t alloc_act(size_t bytes) {
        const size_t o = (top + 4095) & ~(size_t)4095;
        top = o + bytes;
        return o;
    }
    size_t alloc(size_t bytes) {
        tail += (bytes + 255) & ~(size_t)255;
        return end - tail;
    }
    size_t need() const { return ((top + 255) & ~(size_t)255) + tail; }
    void* at(size_t off) const { return base + off; }

    Act new_act(int C, int d, int h, int w, bool fp32 = false) {
        Act a;
        a.C = C; a.D = d; a.H = h; a.W = w;
        a.esize = fp32 ? 4 : half_esize;
        const size_t b = a.bytes(N);
        auto& fr = pool[{b, a.esize}];
        if (!fr.empty()) { a.off = fr.back(); fr.pop_back(); }
        else a.off = alloc_act(b);
        return a;
    }
    void release(const Act& a) { pool[{a.bytes(N), a.esize}].push_back(a.off); }

    // gn_finalize over the virtual concat of srcs; gamma NULL = bounds only (skipped when nothing reads them)
    bool finalize(const Act* s0, const Act* s1, const float* gamma, const float* beta, int film_off, bool force_bound,
                  size_t* A, size_t* B, size_t* bound, bool* has) {
        *has = false;
        if (!gamma && !(scaled || force_bound)) return true;
        if (s1 && s1->voxels() != s0->voxels()) return fail("concat of tensors with different spatial size");
        const int Cn = s0->C + (s1 ? s1->C : 0);
        Step st = new_step(DDPM3D_STEP_FINALIZE);
        ddpm3d_plan_step& r = st.rec;
        r.in[0] = at(s0->stats_off); r.n[0] = s0->C; r.n[1] = s0->rows;
        if (s1) { r.in[1] = at(s1->stats_off); r.n[2] = s1->C; r.n[3] = s1->rows; }
        r.n[4] = N; r.n[5] = 32;
        r.count = (double)s0->voxels(); r.eps = 1e-5f;
        r.in[2] = gamma; r.in[3] = beta;
        *A = *B = 0;
        if (gamma) {
            *A = alloc((size_t)N * Cn * 4); *B = alloc((size_t)N * Cn * 4);
            r.out[0] = at(*A); r.out[1] = at(*B);
        }
        *bound = alloc((size_t)N * 32 * 2 * 4);
        r.out[2] = at(*bound);
        if (film_off >= 0) { r.flags = DDPM3D_STEP_FILM; r.film_off = film_off; }
        steps.push_back(st);
        *has = true;
        return true;
    }

    struct ConvArgs {
        const Act* src0 = nullptr; const Act* src1 = nullptr;
        Act* out = nullptr;
        size_t A = 0, B = 0; bool aff = false;
        int act = DDPM3D_ACT_NONE, in_mode = DDPM3D_IN_SAME;
        const Act* res = nullptr; int res_mode = DDPM3D_RES_NONE;
        bool planar = false, want_stats = true, bias_per_n = false;
        bool ncdhw_out = false;                    // the network's last conv: out pointer patched per call
        size_t bound = 0; int bound_first = 0, bound_count = 0, bound_stride = 0; bool has_bound = false;
        int film_off = 0;
        // the ResBlock tail as ONE ddpm3d_conv3d_skip step where the library takes its fused form: the 1x1 conv, its
        // sources and the first entry of their bound (count / stride as `bound`); *fused = false, and nothing
        // planned, where it does not
        const ddpm3d_conv_weights* skip_w = nullptr;
        const Act* x0 = nullptr; const Act* x1 = nullptr;
        size_t xbound = 0; int xbound_first = 0; bool has_xbound = false;
        bool* fused = nullptr;
    };
    bool conv_step(const ddpm3d_conv_weights& pc, ConvArgs a) {
        ddpm3d_conv_desc d;
        memset(&d, 0, sizeof(d));
        const bool wz = pc.w_packed_wz && !a.planar && (a.in_mode == DDPM3D_IN_SAME || a.in_mode == DDPM3D_IN_UP);
        d.precision = wz ? (pc.precision_wz & ~DDPM3D_WZ_UP_PHASE_IMAGE) : (pc.precision & ~DDPM3D_SKIP_TWO_CALLS);
        d.w_packed = wz ? pc.w_packed_wz : pc.w_packed;
        // a phase image (ddpm3d_pack_up_phase_weight) starts with the plain Winograd-D image: its IN_UP calls run the
        // four-phase form where the library finds the shape fit (ddpm3d.h DDPM3D_HINT_UP_PHASE), the others as ever
        if (wz && (pc.precision_wz & DDPM3D_WZ_UP_PHASE_IMAGE) && a.in_mode == DDPM3D_IN_UP)
            d.kernel_hint = DDPM3D_HINT_UP_PHASE;
        d.bias = pc.bias;
        d.Cout = pc.Cout; d.ksize = pc.ksize;
        const Act* geo = a.out ? a.out : a.src0;
        d.N = N; d.D = geo->D; d.H = geo->H; d.W = geo->W;
        d.out_layout = a.ncdhw_out ? DDPM3D_OUT_NCDHW : DDPM3D_OUT_NDHWC;
        if (a.planar) {
            d.in_mode = DDPM3D_IN_PLANAR2; d.Cin = 2; d.C0 = 1; d.C1 = 1;
        } else {
            d.in_mode = a.in_mode;
            d.src0 = (const float*)at(a.src0->off); d.C0 = a.src0->C;
            if (a.src1) { d.src1 = (const float*)at(a.src1->off); d.C1 = a.src1->C; }
            d.Cin = d.C0 + d.C1;
            if (d.Cin != pc.Cin) return fail("conv %dx%d fed %d channels", pc.Cout, pc.Cin, d.Cin);
            if (a.src0->esize == 2) d.io_dtype |= DDPM3D_IO_SRC0_BF16;
            if (a.src1 && a.src1->esize == 2) d.io_dtype |= DDPM3D_IO_SRC1_BF16;
        }
        if (a.out) {
            d.out = (float*)at(a.out->off);
            if (a.out->esize == 2) d.io_dtype |= DDPM3D_IO_OUT_BF16;
        }
        if (a.aff) { d.aff_a = (const float*)at(a.A); d.aff_b = (const float*)at(a.B); }
        d.act = a.act;
        if (a.res) {
            if (a.res->C != pc.Cout) return fail("residual has %d channels, the conv writes %d", a.res->C, pc.Cout);
            d.res = (const float*)at(a.res->off);
            if (a.res->esize == 2) d.io_dtype |= DDPM3D_IO_RES_BF16;
        }
        d.res_mode = a.res_mode;
        if (d.io_dtype && f16) d.io_dtype |= DDPM3D_IO_HALF_IS_F16;
        if (scaled) {
            if (!a.has_bound) return fail("conv step without an input bound");
            d.in_bound = (const float*)at(a.bound) + a.bound_first;
            d.in_bound_count = a.bound_count; d.in_bound_stride = a.bound_stride;
        }
        ddpm3d_conv_skip sk;
        memset(&sk, 0, sizeof(sk));
        if (a.skip_w) {
            sk.src0 = (const float*)at(a.x0->off); sk.C0 = a.x0->C;
            if (a.x1) { sk.src1 = (const float*)at(a.x1->off); sk.C1 = a.x1->C; }
            sk.w_packed = a.skip_w->w_packed; sk.bias = a.skip_w->bias;
            if (a.x0->esize == 2) sk.io_dtype |= DDPM3D_IO_SRC0_BF16;
            if (a.x1 && a.x1->esize == 2) sk.io_dtype |= DDPM3D_IO_SRC1_BF16;
            if (scaled) {
                if (!a.has_xbound) return fail("skip conv without an input bound");
                sk.in_bound = (const float*)at(a.xbound) + a.xbound_first;
                sk.in_bound_count = a.bound_count; sk.in_bound_stride = a.bound_stride;
            }
            *a.fused = ddpm3d_conv_skip_fused(&d, &sk) != 0;
            if (!*a.fused) return true;
        }
        // how the library itself will run this descriptor: statistics rows, split-K scratch (needs real-looking
        // pointers only where the validation looks at them: none while sizing)
        int rows = 0, split = 1;
        size_t need = 0;
        const int rc = ddpm3d_conv_plan(&d, &rows, &need, &split);
        if (rc != DDPM3D_OK) { code = rc; return fail("%s", ddpm3d_last_error()); }
        if (a.out && a.want_stats) {
            a.out->rows = rows;
            a.out->stats_off = alloc((size_t)N * rows * pc.Cout * 2 * sizeof(double));
            d.stats = (double*)at(a.out->stats_off);
            d.stats_rows = rows;
        }
        if (need) { ws_steps.push_back((int)steps.size()); if (need > ws_bytes) ws_bytes = need; }
        // (rec.conv / rec.skip are set once the list has stopped growing: ddpm3d_unet_plan_create)
        Step st = new_step(DDPM3D_STEP_CONV);
        st.conv = d;
        st.skip = sk;                              // all zero where the step is a plain ddpm3d_conv3d call
        st.rec.flags = (a.planar ? DDPM3D_STEP_X | DDPM3D_STEP_LOW_RES : 0) | (a.ncdhw_out ? DDPM3D_STEP_OUT : 0) |
                       (a.bias_per_n ? DDPM3D_STEP_FILM_BIAS : 0);
        st.rec.film_off = a.bias_per_n ? a.film_off : 0;
        steps.push_back(st);
        return true;
    }

    bool resblock(const ddpm3d_layer& e, const Act* s0, const Act* s1, Act* y_out) {
        int d = s0->D, h = s0->H, w = s0->W, im = DDPM3D_IN_SAME, rm = DDPM3D_RES_SAME;
        if (e.updown == DDPM3D_UPDOWN_DOWN) {
            if ((s0->H | s0->W) & 1) return fail("Downsample needs even H, W (got %dx%d)", s0->H, s0->W);
            h /= 2; w /= 2; im = DDPM3D_IN_POOL; rm = DDPM3D_RES_POOL;
        } else if (e.updown == DDPM3D_UPDOWN_UP) {
            h *= 2; w *= 2; im = DDPM3D_IN_UP; rm = DDPM3D_RES_UP;
        }
        size_t A1, B1, bnd1; bool has1;
        if (!finalize(s0, s1, e.norm1_gamma, e.norm1_beta, -1, false, &A1, &B1, &bnd1, &has1)) return false;
        Act h1 = new_act(e.conv1.Cout, d, h, w);
        ConvArgs c1;
        c1.src0 = s0; c1.src1 = s1; c1.out = &h1; c1.A = A1; c1.B = B1; c1.aff = true; c1.act = DDPM3D_ACT_SILU;
        c1.in_mode = im; c1.bound = bnd1; c1.bound_first = 0; c1.bound_count = 32; c1.bound_stride = 2; c1.has_bound = has1;
        Act pooled;
        bool use_pooled = false;
        if (e.updown == DDPM3D_UPDOWN_DOWN && e.conv1.w_packed_wz && !s1) {
            // h_upd(in_rest(x)) as a pass of its own: conv1 then reads a plain tensor and runs its Winograd-D form
            pooled = new_act(s0->C, d, h, w, true);
            Step st = new_step(DDPM3D_STEP_POOL_ACT);
            ddpm3d_plan_step& r = st.rec;
            r.in[0] = at(s0->off); r.in[1] = at(A1); r.in[2] = at(B1);
            r.n[0] = DDPM3D_ACT_SILU; r.n[1] = 1; r.n[2] = N; r.n[3] = d; r.n[4] = h; r.n[5] = w; r.n[6] = s0->C;
            r.out[0] = at(pooled.off);
            r.n[7] = (s0->esize == 2 ? DDPM3D_IO_SRC0_BF16 : 0) | ((s0->esize == 2 && f16) ? DDPM3D_IO_HALF_IS_F16 : 0);
            steps.push_back(st);
            c1.src0 = &pooled; c1.aff = false; c1.act = DDPM3D_ACT_NONE; c1.in_mode = DDPM3D_IN_SAME;
            use_pooled = true;
        }
        size_t A2, B2, bnd2; bool has2;
        if (m.film) {
            if (!conv_step(e.conv1, c1)) return false;
            if (!finalize(&h1, nullptr, e.norm2_gamma, e.norm2_beta, e.film_off, false, &A2, &B2, &bnd2, &has2)) return false;
        } else {
            c1.bias_per_n = true; c1.film_off = e.film_off;     // additive embedding: conv1's bias is the film row slice
            if (!conv_step(e.conv1, c1)) return false;
            if (!finalize(&h1, nullptr, e.norm2_gamma, e.norm2_beta, -1, false, &A2, &B2, &bnd2, &has2)) return false;
        }
        if (use_pooled) release(pooled);
        Act y = new_act(e.conv2.Cout, d, h, w);
        ConvArgs c2;
        c2.src0 = &h1; c2.out = &y; c2.A = A2; c2.B = B2; c2.aff = true; c2.act = DDPM3D_ACT_SILU;
        c2.bound = bnd2; c2.bound_count = 32; c2.bound_stride = 2; c2.has_bound = has2;
        if (e.skip.w_packed) {
            if (e.updown != DDPM3D_UPDOWN_NONE) return fail("up/down ResBlock with a channel change is not in the reference");
            // y = skip(x) on the RAW block input (its range: entry 1 of the same finalize) -- in ONE step where the
            // library runs the 1x1 conv inside conv2's launch (ddpm3d_conv3d_skip), else -- or where the description
            // carries DDPM3D_SKIP_TWO_CALLS -- as two
            bool fused = false;
            if (!(e.skip.precision & DDPM3D_SKIP_TWO_CALLS)) {
                ConvArgs cf = c2;
                cf.skip_w = &e.skip; cf.x0 = s0; cf.x1 = s1;
                cf.xbound = bnd1; cf.xbound_first = 1; cf.has_xbound = has1; cf.fused = &fused;
                if (!conv_step(e.conv2, cf)) return false;
            }
            if (fused) {
                release(h1);
                *y_out = y;
                return true;
            }
            ConvArgs cs;
            cs.src0 = s0; cs.src1 = s1; cs.out = &y; cs.want_stats = false;
            cs.bound = bnd1; cs.bound_first = 1; cs.bound_count = 32; cs.bound_stride = 2; cs.has_bound = has1;
            if (!conv_step(e.skip, cs)) return false;
            c2.res = &y; c2.res_mode = DDPM3D_RES_SAME;
        } else {
            if (s1) return fail("ResBlock with an Identity skip over a concatenated input (%d + %d -> %d channels)",
                                s0->C, s1->C, e.conv2.Cout);
            c2.res = s0; c2.res_mode = rm;
        }
        if (!conv_step(e.conv2, c2)) return false;
        release(h1);
        *y_out = y;
        return true;
    }

    bool attention(const ddpm3d_layer& e, const Act* x, Act* y_out) {
        const int Cn = x->C;
        if (e.heads <= 0 || Cn % e.heads) return fail("attention: %d channels not divisible by %d heads", Cn, e.heads);
        const int ch = Cn / e.heads;
        if (ch != 32 && ch != 64 && ch != 128) return fail("attention with %d channels per head (32, 64 or 128 are built)", ch);
        size_t A, B, bnd; bool has;
        if (!finalize(x, nullptr, e.norm1_gamma, e.norm1_beta, -1, false, &A, &B, &bnd, &has)) return false;
        Act qkv = new_act(3 * Cn, x->D, x->H, x->W, true);
        ConvArgs cq;
        cq.src0 = x; cq.out = &qkv; cq.A = A; cq.B = B; cq.aff = true; cq.act = DDPM3D_ACT_NONE;
        cq.bound = bnd; cq.bound_count = 32; cq.bound_stride = 2; cq.has_bound = has;
        if (!conv_step(e.conv1, cq)) return false;
        size_t qA, qB, qb; bool hasq;
        if (!finalize(&qkv, nullptr, nullptr, nullptr, -1, m.arithmetic != DDPM3D_PREC_F32, &qA, &qB, &qb, &hasq)) return false;
        Act a = new_act(Cn, x->D, x->H, x->W, true);
        Step st = new_step(DDPM3D_STEP_ATTENTION);
        ddpm3d_plan_step& r = st.rec;
        r.in[0] = at(qkv.off); r.n[0] = N; r.n[1] = x->voxels(); r.n[2] = e.heads; r.n[3] = ch;
        r.n[4] = m.arithmetic == DDPM3D_PREC_F32 ? DDPM3D_PREC_F32 : DDPM3D_PREC_F16X3;
        if (hasq) r.in[1] = (const float*)at(qb) + 1;
        r.n[5] = 32; r.n[6] = 2;
        r.out[0] = at(a.off);
        steps.push_back(st);
        release(qkv);
        Act y = new_act(Cn, x->D, x->H, x->W);
        ConvArgs cp;
        cp.src0 = &a; cp.out = &y; cp.res = x; cp.res_mode = DDPM3D_RES_SAME;
        cp.bound = qb; cp.bound_first = 1; cp.bound_count = 32; cp.bound_stride = 2; cp.has_bound = hasq;
        if (!conv_step(e.conv2, cp)) return false;
        release(a);
        *y_out = y;
        return true;
    }

    bool layer(const ddpm3d_layer& e, const Act* s0, const Act* s1, Act* out) {
        // a description with a hole in it is refused here, not discovered by a kernel
        const bool n1 = e.norm1_gamma && e.norm1_beta, n2 = e.norm2_gamma && e.norm2_beta;
        const bool c1 = e.conv1.w_packed && e.conv1.bias, c2 = e.conv2.w_packed && e.conv2.bias;
        if (e.kind == DDPM3D_LAYER_RES && !(n1 && n2 && c1 && c2 && (!e.skip.w_packed || e.skip.bias)))
            return fail("ResBlock description without its norms / convs");
        if (e.kind == DDPM3D_LAYER_ATTN && !(n1 && c1 && c2)) return fail("AttentionBlock description without norm / qkv / proj_out");
        if ((e.kind == DDPM3D_LAYER_UPCONV || e.kind == DDPM3D_LAYER_DOWNCONV) && !c1) return fail("resampling conv without weights");
        if (e.kind == DDPM3D_LAYER_RES) return resblock(e, s0, s1, out);
        if (e.kind == DDPM3D_LAYER_ATTN) return attention(e, s0, out);
        if (e.kind == DDPM3D_LAYER_UPCONV || e.kind == DDPM3D_LAYER_DOWNCONV) {
            const bool up = e.kind == DDPM3D_LAYER_UPCONV;
            if (!up && ((s0->H | s0->W) & 1)) return fail("Downsample needs even H, W (got %dx%d)", s0->H, s0->W);
            Act y = new_act(e.conv1.Cout, s0->D, up ? s0->H * 2 : s0->H / 2, up ? s0->W * 2 : s0->W / 2);
            size_t A, B, bnd; bool has;
            if (!finalize(s0, nullptr, nullptr, nullptr, -1, false, &A, &B, &bnd, &has)) return false;
            ConvArgs c;
            c.src0 = s0; c.out = &y; c.in_mode = up ? DDPM3D_IN_UP : DDPM3D_IN_STRIDE2;
            c.bound = bnd; c.bound_first = 1; c.bound_count = 32; c.bound_stride = 2; c.has_bound = has;
            if (!conv_step(e.conv1, c)) return false;
            *out = y;
            return true;
        }
        return fail("unknown layer kind %d", e.kind);
    }

    // range of the network input (it carries no statistics): max |x| [, max |low_res|] per sample
    void absmax_step(size_t per_sample, int flags) {
        Step st = new_step(DDPM3D_STEP_ABSMAX);
        st.rec.flags = flags;
        st.rec.n[0] = N; st.rec.n[1] = (int64_t)per_sample;
        st.rec.out[0] = at(in_absmax);
        if (scaled) steps.push_back(st);
    }

    bool build() {
        // the block tables are what the loops below index `layers` and the skip stack with: refuse a table that
        // does not cover exactly n_layers, or that pops more skips than the encoder pushes, before any indexing
        long long covered = m.n_middle_layers;
        bool tables = m.n_input_blocks >= 0 && m.n_middle_layers >= 0 && m.n_output_blocks >= 0;
        for (int b = 0; tables && b < m.n_input_blocks; ++b) { tables = m.input_block_layers[b] >= 0; covered += m.input_block_layers[b]; }
        for (int b = 0; tables && b < m.n_output_blocks; ++b) { tables = m.output_block_layers[b] >= 0; covered += m.output_block_layers[b]; }
        if (!tables || covered != m.n_layers) return fail("the block sizes cover %lld of %d layers", covered, m.n_layers);
        if (m.n_output_blocks > m.n_input_blocks + 1)
            return fail("%d output blocks for %d input blocks: nothing left on the skip stack", m.n_output_blocks, m.n_input_blocks + 1);
        Act h = new_act(m.first.Cout, D, H, W);
        Act xin;
        if (m.planar) {
            in_absmax = alloc((size_t)N * 2 * 4);
            absmax_step((size_t)D * H * W, DDPM3D_STEP_X | DDPM3D_STEP_LOW_RES);
            ConvArgs c;
            c.out = &h; c.planar = true; c.bound = in_absmax; c.bound_count = 2; c.bound_stride = 1; c.has_bound = true;
            if (!conv_step(m.first, c)) return false;
        } else {
            xin = new_act(m.cin_pad, D, H, W, true);
            in_absmax = alloc((size_t)N * 4);
            absmax_step((size_t)m.in_channels * D * H * W, DDPM3D_STEP_X);
            Step sp = new_step(DDPM3D_STEP_PAD);
            sp.rec.flags = DDPM3D_STEP_X;
            sp.rec.n[0] = N; sp.rec.n[1] = m.in_channels; sp.rec.n[2] = D * H * W; sp.rec.n[3] = m.cin_pad;
            sp.rec.out[0] = at(xin.off);
            steps.push_back(sp);
            ConvArgs c;
            c.src0 = &xin; c.out = &h; c.bound = in_absmax; c.bound_count = 1; c.bound_stride = 1; c.has_bound = true;
            if (!conv_step(m.first, c)) return false;
        }
        std::vector<Act> hs;
        hs.push_back(h);
        int li = 0;
        for (int b = 0; b < m.n_input_blocks; ++b) {
            for (int i = 0; i < m.input_block_layers[b]; ++i) {
                Act prev = h;
                if (!layer(m.layers[li++], &prev, nullptr, &h)) return false;
                if (i > 0) release(prev);          // a block's intermediate; its input stays on the skip stack
            }
            hs.push_back(h);
        }
        for (int i = 0; i < m.n_middle_layers; ++i) {
            Act prev = h;
            if (!layer(m.layers[li++], &prev, nullptr, &h)) return false;
            if (prev.off != hs.back().off) release(prev);
        }
        for (int b = 0; b < m.n_output_blocks; ++b) {
            Act skip = hs.back();
            hs.pop_back();
            Act s0 = h, s1 = skip;
            bool two = true;
            for (int i = 0; i < m.output_block_layers[b]; ++i) {
                if (!layer(m.layers[li++], &s0, two ? &s1 : nullptr, &h)) return false;
                release(s0);
                // (without a middle block the first output block reads ONE tensor as input and as skip)
                if (two && s1.off != s0.off) release(s1);
                s0 = h;
                two = false;
            }
        }
        size_t A, B, bnd; bool has;
        if (!finalize(&h, nullptr, m.out_gamma, m.out_beta, -1, false, &A, &B, &bnd, &has)) return false;
        ConvArgs c;
        c.src0 = &h; c.A = A; c.B = B; c.aff = true; c.act = DDPM3D_ACT_SILU; c.ncdhw_out = true; c.want_stats = false;
        c.bound = bnd; c.bound_count = 32; c.bound_stride = 2; c.has_bound = has;
        if (!conv_step(m.out, c)) return false;
        release(h);
        if (ws_bytes) ws_off = alloc_act(ws_bytes);
        for (int i : ws_steps) { steps[i].conv.workspace = at(ws_off); steps[i].conv.workspace_bytes = ws_bytes; }
        return true;
    }
};

thread_local char g_unet_err[256] = "";

}  // namespace

struct ddpm3d_unet_plan {
    std::vector<Step> steps;     // never resized: the conv records point into it
    int planar;
};

extern "C" {

const char* ddpm3d_unet_last_error(void) { return g_unet_err; }

static bool desc_ok(const ddpm3d_unet_desc* m, int N, int D, int H, int W) {
    return m && N > 0 && D > 0 && H > 0 && W > 0 && m->layers && m->n_layers > 0 && m->first.w_packed && m->out.w_packed &&
           m->out_gamma && m->out_beta && (m->n_input_blocks == 0 || m->input_block_layers) &&
           (m->n_output_blocks == 0 || m->output_block_layers) &&
           (m->arithmetic == DDPM3D_PREC_F32 || m->arithmetic == DDPM3D_PREC_F16X3 || m->arithmetic == DDPM3D_PREC_F16 ||
            m->arithmetic == DDPM3D_PREC_BF16);
}

size_t ddpm3d_unet_plan_bytes(const ddpm3d_unet_desc* m, int N, int D, int H, int W) {
    if (!desc_ok(m, N, D, H, W)) { snprintf(g_unet_err, sizeof(g_unet_err), "unet_plan_bytes: bad description"); return 0; }
    // sizing pass: the same planning against a base that is never dereferenced (non-null, so that the per-op
    // validation sees what it will see at run time)
    Planner p(*m, N, D, H, W, reinterpret_cast<char*>(4096), (size_t)1 << 46);
    if (!p.build()) { snprintf(g_unet_err, sizeof(g_unet_err), "%s", p.err); return 0; }
    return p.need();
}

int ddpm3d_unet_plan_create(const ddpm3d_unet_desc* m, int N, int D, int H, int W, void* arena, size_t arena_bytes,
                            ddpm3d_unet_plan** plan) {
    if (!desc_ok(m, N, D, H, W) || !arena || !plan || (reinterpret_cast<uintptr_t>(arena) & 255)) {
        snprintf(g_unet_err, sizeof(g_unet_err), "unet_plan_create: bad description, or an arena that is not 256-byte aligned");
        return DDPM3D_EINVAL;
    }
    // (the small buffers are carved from the arena's end: size the plan before any address is formed)
    const size_t need = ddpm3d_unet_plan_bytes(m, N, D, H, W);
    if (need > arena_bytes) {
        snprintf(g_unet_err, sizeof(g_unet_err), "unet_plan_create: the plan needs %zu bytes, the arena has %zu", need, arena_bytes);
        return DDPM3D_EINVAL;
    }
    Planner p(*m, N, D, H, W, static_cast<char*>(arena), arena_bytes);
    if (!p.build()) { snprintf(g_unet_err, sizeof(g_unet_err), "%s", p.err); return p.code; }
    ddpm3d_unet_plan* pl = new (std::nothrow) ddpm3d_unet_plan();
    if (!pl) return DDPM3D_EINVAL;
    pl->steps.swap(p.steps);
    for (Step& s : pl->steps)
        if (s.rec.kind == DDPM3D_STEP_CONV) { s.rec.conv = &s.conv; s.rec.skip = s.skip.w_packed ? &s.skip : nullptr; }
    pl->planar = m->planar;
    *plan = pl;
    return DDPM3D_OK;
}

void ddpm3d_unet_plan_destroy(ddpm3d_unet_plan* plan) { delete plan; }

int ddpm3d_unet_plan_steps(ddpm3d_unet_plan* pl, ddpm3d_plan_step* out, int capacity) {
    if (!pl) { snprintf(g_unet_err, sizeof(g_unet_err), "unet_plan_steps: no plan"); return DDPM3D_EINVAL; }
    const int n = (int)pl->steps.size();
    for (int i = 0; out && i < n && i < capacity; ++i) out[i] = pl->steps[i].rec;
    return n;
}

// one call of the list, with what belongs to this forward patched in (ddpm3d.h: DDPM3D_STEP_* flags)
static int issue(const ddpm3d_plan_step& s, const float* x, const float* low_res, const float* film_rows, int film_stride,
                 float* out, void* stream) {
    const bool film = s.flags & DDPM3D_STEP_FILM;
    const float* lr = (s.flags & DDPM3D_STEP_LOW_RES) ? low_res : nullptr;
    switch (s.kind) {
        case DDPM3D_STEP_CONV: {
            ddpm3d_conv_desc& d = *s.conv;
            if (s.flags & DDPM3D_STEP_X) d.src0 = x;
            if (s.flags & DDPM3D_STEP_LOW_RES) d.src1 = low_res;
            if (s.flags & DDPM3D_STEP_OUT) d.out = out;
            if (s.flags & DDPM3D_STEP_FILM_BIAS) { d.bias = film_rows + s.film_off; d.bias_stride_n = film_stride; }
            return s.skip ? ddpm3d_conv3d_skip(&d, s.skip, stream) : ddpm3d_conv3d(&d, stream);
        }
        case DDPM3D_STEP_FINALIZE:
            return ddpm3d_gn_finalize((const double*)s.in[0], (int)s.n[0], (int)s.n[1], (const double*)s.in[1], (int)s.n[2],
                                      (int)s.n[3], (int)s.n[4], (int)s.n[5], s.count, s.eps, (const float*)s.in[2],
                                      (const float*)s.in[3], film ? film_rows : nullptr, film ? film_stride : 0, s.film_off,
                                      (float*)s.out[0], (float*)s.out[1], (float*)s.out[2], stream);
        case DDPM3D_STEP_ABSMAX: return ddpm3d_absmax(x, lr, (int)s.n[0], (size_t)s.n[1], (float*)s.out[0], stream);
        case DDPM3D_STEP_PAD:
            return ddpm3d_ncdhw_to_ndhwc_pad(x, (int)s.n[0], (int)s.n[1], (int)s.n[2], (int)s.n[3], (float*)s.out[0], stream);
        case DDPM3D_STEP_POOL_ACT:
            return ddpm3d_pool_act(s.in[0], (const float*)s.in[1], (const float*)s.in[2], (int)s.n[0], (int)s.n[1], (int)s.n[2],
                                   (int)s.n[3], (int)s.n[4], (int)s.n[5], (int)s.n[6], s.out[0], (int)s.n[7], stream);
        case DDPM3D_STEP_ATTENTION:
            return ddpm3d_attention_p((const float*)s.in[0], (int)s.n[0], (int)s.n[1], (int)s.n[2], (int)s.n[3], (int)s.n[4],
                                      (const float*)s.in[1], (int)s.n[5], (int)s.n[6], (float*)s.out[0], stream);
    }
    return DDPM3D_EINVAL;
}

int ddpm3d_unet_forward(ddpm3d_unet_plan* pl, const float* x, const float* low_res, const float* film_rows,
                        int film_stride, float* out, void* stream) {
    if (!pl || !x || !film_rows || !out || (pl->planar && !low_res)) {
        snprintf(g_unet_err, sizeof(g_unet_err), "unet_forward: null argument");
        return DDPM3D_EINVAL;
    }
    for (const Step& s : pl->steps) {
        const int rc = issue(s.rec, x, low_res, film_rows, film_stride, out, stream);
        if (rc != DDPM3D_OK) {
            snprintf(g_unet_err, sizeof(g_unet_err), "unet_forward: %s", ddpm3d_last_error());
            return rc;
        }
    }
    return DDPM3D_OK;
}

}  // extern "C"
