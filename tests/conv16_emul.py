"""
CPU emulation of the 16-bit convolution arithmetic (precisions 2, 4, 5, 6 of include/ddpm3d.h), for the tests.

Plain torch / numpy, evaluated in fp64 except where a kernel rounds; each rounding below names the kernel line
it mirrors.  What is NOT emulated: the order of the fp32 accumulation, and the fast SiLU (v_exp_f32 / v_rcp_f32,
a few ulp).  The emulator instead returns, per output element, the quantities a bound on those two needs:

  absterms  sum of |terms| (products, transform terms, bias, residual) -- the classical summation bound;
  sqterms   sum over the accumulators of (sum of squared products + accumulator^2): the variance scale of the
            fp32 rounding errors along an accumulation (see test_gpu_conv16.py for the derivation);
  flip      sum over the operands whose 16-bit rounding the fast SiLU can change (its fp32 value lies within
            `delta` of a rounding boundary) of one 16-bit ulp times |weight|: a rigorous bound on what those
            flips move the output by.

Inputs are NCDHW tensors in their storage dtype (fp32, f16 or bf16: read exactly); outputs NCDHW fp64.
"""

import math

import numpy as np
import torch
import torch.nn.functional as F

W_TARGET = 8.0        # DDPM3D_X3_W_TARGET (csrc/conv3d_params.h:16)
F16_MODES = (2, 4)
WZ_MODES = (4, 6)


class Rounding:
    """The rounding points.  exact=True switches every one of them off (fp64 throughout)."""

    def __init__(self, precision, exact=False, mode="rne", round_ops=True):
        self.f16 = precision in F16_MODES
        self.exact = exact
        self.mode = mode              # "rne", or "trunc" (a mutation: truncation toward zero)
        self.round_ops = round_ops and not exact

    def r32(self, x):
        return x if self.exact else x.float().double()

    def r16(self, x):
        """16-bit rounding of fp64 tensors that hold fp32 values: f16 (np.float16, subnormals included) or bf16."""
        if not self.round_ops:
            return x
        x32 = x.float()
        if self.f16:
            h = x32.numpy().astype(np.float16)
            if self.mode == "trunc":
                over = np.abs(h.astype(np.float64)) > np.abs(x32.numpy().astype(np.float64))
                h = np.where(over, np.nextafter(h, np.float16(0)), h)
            return torch.from_numpy(h.astype(np.float64))
        if self.mode == "trunc":
            return (x32.view(torch.int32) & -65536).view(torch.float32).double()
        return x32.bfloat16().double()


def fma32(x, a, b):
    """fmaf(x, a, b) on fp32 values held in fp64: the product is exact in fp64, the sum is rounded once to fp32
    (conv3d_load.h:27 / :217, conv3d_stage.h:196, conv3d_skinny.hip:152).  A sum that lands on an fp32 tie
    after its fp64 rounding is resolved from the exact tail (TwoSum), so there is no double rounding."""
    p = x * a
    s = p + b
    bb = s - p
    tail = (p - (s - bb)) + (b - bb)
    r = s.float().double()
    up = torch.nextafter(r.float(), torch.full_like(r.float(), float("inf"))).double()
    dn = torch.nextafter(r.float(), torch.full_like(r.float(), float("-inf"))).double()
    tie = ((s - r).abs() * 2 == torch.where(s > r, up - r, r - dn)) & (tail != 0)
    s = torch.where(tie, s + tail.sign() * (s - r).abs() * 0.5, s)
    return s.float().double()


def act_scale(bound, gain):
    """act_scale_finish (conv3d_load.h:229): S = 2^(14 - floor(log2(gain * max bound))), k clamped to +-60."""
    b = float(np.float32(np.float32(np.max(bound)) * np.float32(gain)))
    if not (b > 0) or not math.isfinite(b):
        return 1.0
    k = 14 - (math.frexp(b)[1] - 1)
    return 2.0 ** max(-60, min(60, k))


def weight_scale(wmax):
    """pack_scale_kernel (ops.hip), whatever the weight source: s = 2^floor(log2(W_TARGET / max|w|)),
    clamped to [2^-24, 2^24]; 1 for an all-zero channel."""
    m = float(wmax)
    if not (m > 0 and m < 3.0e38):
        return 1.0
    q = float(np.float32(W_TARGET) / np.float32(m))
    return 2.0 ** max(-24, min(24, math.floor(math.log2(q))))


def _silu(y, rnd, sig_scale, act):
    """silu_f<true> (conv3d_load.h:17) / the exp2-rcp form (conv3d_stage.h:200): v = y * sigmoid(y), the
    sigmoid exact and rounded to fp32, the product rounded to fp32.  delta bounds |kernel - this| per value:
    v_exp_f32 and v_rcp_f32 (1 ulp each), the rounded exponent argument and log2(e) (|y| * 2^-24 each), 1 + e
    and the product (half an ulp each) on the kernel's side; the two roundings here (half an ulp each)."""
    if not act:
        return y, torch.zeros_like(y)
    sig = rnd.r32(torch.sigmoid(y) * sig_scale)
    v = rnd.r32(y * sig)
    delta = 2.0 ** -24 * (8.0 + 2.0 * y.abs()) * v.abs()
    return v, delta


def _flip(rnd, xs, ds):
    """one 16-bit ulp where the kernel's value (within ds of xs) can round differently, else 0"""
    if not rnd.round_ops:
        return torch.zeros_like(xs)
    return (rnd.r16(xs + ds) - rnd.r16(xs - ds)).abs()


def _pool(t, exact):
    """AvgPool3d((1,2,2)) in the kernel's order, fp32: ((s00 + s01) + s10) + s11, then * 1/4 (conv3d_load.h:150)."""
    r = (lambda z: z) if exact else (lambda z: z.float().double())
    s00, s01 = t[..., 0::2, 0::2], t[..., 0::2, 1::2]
    s10, s11 = t[..., 1::2, 0::2], t[..., 1::2, 1::2]
    return r(r(r(s00 + s01) + s10) + s11) * 0.25


def _up(t):
    return t.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


def conv16(srcs, w, b, precision, in_mode="same", aff=None, act=False, bound=None, res=None, res_mode="none",
           out16=False, exact=False, round_mode="rne", round_ops=True, round_before_transform=False,
           sig_scale=1.0, use_wscale=True):
    """Emulate ddpm3d_conv3d for precision 2 (f16 direct), 4 (f16 Winograd-D), 5 (bf16 direct), 6 (bf16 Winograd-D).

    srcs: one or two NCDHW tensors (the virtual concat; in_mode "planar": the two single-channel volumes)
    w, b: fp32 OIDHW weights (k = 1 or 3) and bias; aff: (A, B) [N, Cin] fp32; act: SiLU after the affine
    in_mode: "same" | "up" | "pool" | "stride2" | "planar"; res_mode: "none" | "same" | "up" | "pool"
    bound: [N, k] fp32 in_bound entries (split-f16 modes only); out16: round the stored value to f16 / bf16.
    Mutations (for the discrimination tests): round_mode "trunc", round_ops False, round_before_transform,
    sig_scale, use_wscale False.
    Returns a dict of NCDHW fp64 tensors: out, stored, absterms, sqterms, flip; and the scales used."""
    rnd = Rounding(precision, exact=exact, mode=round_mode, round_ops=round_ops)
    x = torch.cat([s.double() for s in srcs], dim=1)
    N, Cin = x.shape[0], x.shape[1]
    Cout, k = w.shape[0], w.shape[2]
    # ---- input as the matrix cores see it, before scaling: v = act(fma(x, A, B)) per source voxel
    if aff is not None and in_mode != "planar":
        A = aff[0].double().reshape(N, Cin, 1, 1, 1)
        B = aff[1].double().reshape(N, Cin, 1, 1, 1)
        y = x * A + B if exact else fma32(x, A.expand_as(x), B.expand_as(x))
    else:
        y = x
    v, delta = _silu(y, rnd, sig_scale, act)
    if in_mode == "up":
        v, delta = _up(v), _up(delta)
    elif in_mode == "pool":
        s_abs = _pool(v.abs(), True)
        v = _pool(v, exact)
        delta = 0.25 * (_pool(delta, True) * 4 + 3 * 2.0 ** -23 * 4 * s_abs) if act else torch.zeros_like(v)
    wz = precision in WZ_MODES
    # ---- the activation scale (split-f16 modes only; the bf16 modes have fp32's exponent range)
    if precision in F16_MODES and not exact:
        S = [act_scale(bound[n].numpy(), 2.0 if wz else 1.0) for n in range(N)]
    else:
        S = [1.0] * N
    Sv = torch.tensor(S, dtype=torch.float64).reshape(N, 1, 1, 1, 1)
    w64 = w.double()
    stride, pad = ((1, 2, 2) if in_mode == "stride2" else 1), k // 2
    if not wz:
        # direct kernels: operand = 16-bit(v * S) (conv3d.hip:174-185, conv1x1.hip:61 pw_operand,
        # conv3d_skinny.hip:150-172; bf16: bf16_pack, no scale); weights = 16-bit(w * s_w) (ops.hip pack_split_kernel)
        vs = v * Sv
        a = rnd.r16(vs) / Sv
        fl = _flip(rnd, vs, delta * Sv) / Sv
        if precision in F16_MODES and use_wscale and not exact:
            sw = torch.tensor([weight_scale(np.abs(w[c].numpy()).max()) for c in range(Cout)], dtype=torch.float64)
        else:
            sw = torch.ones(Cout, dtype=torch.float64)
        sw5 = sw.reshape(Cout, 1, 1, 1, 1)
        wq = rnd.r16(rnd.r32(w64 * sw5)) / sw5
        conv = lambda t, ww: F.conv3d(t, ww, stride=stride, padding=pad)
        out = conv(a, wq)
        absterms = conv(a.abs(), wq.abs())
        sq = conv(a * a, wq * wq) + out * out
        flip = conv(fl, wq.abs())
        tr_abs = torch.zeros_like(out)
    else:
        out, absterms, sq, flip, tr_abs, sw = _winograd(v, delta, Sv, w, rnd, round_before_transform, use_wscale,
                                                       precision, exact)
    # ---- epilogue: acc * wscale * (1/S) + bias (+ residual), fp32 (conv3d_epilogue.h:161-176)
    out = out + b.double().reshape(1, Cout, 1, 1, 1)
    absterms = absterms + b.double().abs().reshape(1, Cout, 1, 1, 1)
    if res_mode != "none":
        r = res.double()
        r = {"same": lambda t: t, "up": _up, "pool": lambda t: _pool(t, exact)}[res_mode](r)
        out = out + r
        absterms = absterms + r.abs()
    stored = rnd.r32(out)
    if out16 and not exact:
        stored = Rounding(precision).r16(stored)     # ddpm3d_act_store / half_pack: RNE (conv3d_epilogue.h:185)
    return dict(out=out, stored=stored, absterms=absterms, sqterms=sq, flip=flip, trabs=tr_abs, S=S, wscale=sw)


def _winograd(v, delta, Sv, w, rnd, before, use_wscale, precision, exact):
    """The Winograd F(2,3)-along-depth form as the algorithm: transformed planes, four (1,3,3) convolutions,
    the output transform.  Output z-pair p reads input planes 2p-1 .. 2p+2 (zero outside the volume)."""
    N, Cin, D, H, W = v.shape
    Cout = w.shape[0]
    P = (D + 1) // 2
    # planes -1 .. 2P: the zero padding in depth
    vp = F.pad(v * Sv, (0, 0, 0, 0, 1, 2 * P + 1 - D))
    dp = F.pad(delta * Sv, (0, 0, 0, 0, 1, 2 * P + 1 - D))
    d = [vp[:, :, j + 2 * torch.arange(P)] for j in range(4)]
    dd = [dp[:, :, j + 2 * torch.arange(P)] for j in range(4)]
    r32 = rnd.r32
    if before:
        d = [rnd.r16(t) for t in d]
        r32 = lambda t: t
    # input transform in stage_write (conv3d_stage.h:219-223): d0-d2, d1+d2, d2-d1, d1-d3 in fp32, then 16-bit
    t = [r32(d[0] - d[2]), r32(d[1] + d[2]), r32(d[2] - d[1]), r32(d[1] - d[3])]
    pairs = [(0, 2), (1, 2), (2, 1), (1, 3)]
    tq, fl = [], []
    for j in range(4):
        dt = dd[pairs[j][0]] + dd[pairs[j][1]]
        dt = dt + 2.0 ** -23 * (t[j].abs() + dt) * (dt > 0)
        tq.append(t[j] if before else rnd.r16(t[j]))
        fl.append(_flip(rnd, t[j], dt))
    tq = [q / Sv for q in tq]
    fl = [f / Sv for f in fl]
    # weight transform wz_weight (ops.hip): U0 = g0, U1 = 0.5*((g0+g2)+g1), U2 = 0.5*((g0+g2)-g1), U3 = g2, fp32
    g = [w[:, :, z].double() for z in range(3)]
    if before:
        g = [rnd.r16(x) for x in g]          # (mutation: 16-bit weights, exact transform)
        U = [g[0], 0.5 * ((g[0] + g[2]) + g[1]), 0.5 * ((g[0] + g[2]) - g[1]), g[2]]
    else:
        g02 = rnd.r32(g[0] + g[2])
        U = [g[0], rnd.r32(0.5 * rnd.r32(g02 + g[1])), rnd.r32(0.5 * rnd.r32(g02 - g[1])), g[2]]
    if precision in F16_MODES and use_wscale and not exact and not before:
        m = torch.stack([u.abs().amax(dim=(1, 2, 3)) for u in U]).amax(dim=0)
        sw = torch.tensor([weight_scale(np.float32(m[c].item())) for c in range(Cout)], dtype=torch.float64)
    else:
        sw = torch.ones(Cout, dtype=torch.float64)
    sw4 = sw.reshape(Cout, 1, 1, 1)
    if not before:
        U = [rnd.r16(rnd.r32(u * sw4)) / sw4 for u in U]     # pack_split_kernel<WzTaps> (ops.hip)
    conv = lambda a, u: F.conv3d(a, u.unsqueeze(2), padding=(0, 1, 1))
    M = [conv(tq[j], U[j]) for j in range(4)]
    Ma = [conv(tq[j].abs(), U[j].abs()) for j in range(4)]
    Mq = [conv(tq[j] * tq[j], U[j] * U[j]) + M[j] * M[j] for j in range(4)]
    Mf = [conv(fl[j], U[j].abs()) for j in range(4)]

    def otr(X, sgn):
        # output transform (conv3d_wz.h:254-257): M0 + M1 + M2, M1 - M2 - M3; interleave the pairs, crop D
        z0 = X[0] + X[1] + X[2]
        z1 = X[1] - X[2] - X[3] if sgn else X[1] + X[2] + X[3]
        o = torch.stack([z0, z1], dim=3).reshape(N, Cout, 2 * P, H, W)
        return o[:, :, :D]

    out = otr(M, True)
    absterms = otr(Ma, False)
    sq = otr(Mq, False)
    flip = otr(Mf, False)
    # |M0| + |M1| + |M2| (|M1| + |M2| + |M3|): what the output transform's two fp32 additions round
    tr_abs = otr([m.abs() for m in M], False)
    return out, absterms, sq, flip, tr_abs, sw
