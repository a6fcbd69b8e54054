"""
CPU emulation of the fp32-grade convolution arithmetic (precisions 0, 1, 3 of include/ddpm3d.h), for the tests.

  0  f32: fp32 operands, exact products (v_mfma_f32_32x32x2_f32), the exact SiLU (silu_f<false>).
  1  f16x3, direct / 1x1 / last-layer kernels: the input times the per-sample activation scale S (gain 1) and the
     weights times the per-cout weight scale are each split x = hi + lo, hi = f16(x), lo = f16(x - hi); a product
     is hi*hi + hi*lo + lo*hi (lo*lo is not computed); the fast SiLU (silu_f<true>, v_exp_f32 / v_rcp_f32).
  3  f16x3 on the Winograd F(2,3)-along-depth form: the same split, applied to the fp32 input transform of the
     scaled, activated planes (activation scale gain 2: the transform adds two planes) and to the fp32 weight
     transform made at pack time; the output transform in fp32 in the epilogue.

Plain torch / numpy, fp64 except where a kernel rounds; products are exact and sums fp64.  Reuses
conv16_emul's pieces (fma32, act_scale, weight_scale, _pool, _up).  What is NOT emulated: the order of the fp32
accumulation and the SiLU's last ulps (expf / v_exp_f32, the reciprocal).  The emulator returns, per output
element, what a bound on those needs (see test_gpu_conv32.py):

  absterms  sum of |terms| (products, transform terms, bias, residual);
  sqterms   sum over the accumulators an output combines of (sum of squared products + accumulator^2);
  trabs     |M0| + |M1| + |M2| (|M1| + |M2| + |M3|): what the Winograd output transform's two additions round;
  silu      a rigorous bound on what the SiLU's error moves the output by: the SiLU moves an operand by at most
            `delta`; in the split modes the split then re-rounds lo, by at most one f16 ulp of lo (lo's own
            rounding and the kernel's), and where hi itself can round the other way the weight's lo meets the
            other hi: sum of (delta + ulp(lo)) * |w_hi| + hi-flip * |w_lo| over the operands.  Zero without an
            activation.

Inputs are NCDHW fp32 tensors (fp32 is the only storage the fp32-grade modes read); outputs NCDHW fp64.
"""

import numpy as np
import torch
import torch.nn.functional as F

from conv16_emul import _pool, _up, act_scale, fma32, weight_scale

SPLIT_MODES = (1, 3)
WZ_MODES = (3,)


def r32(x):
    return x.float().double()


def f16(x):
    """RNE to f16 (subnormals included, beyond 65504 -> inf as v_cvt_f16_f32) of fp64 tensors holding fp32 values"""
    with np.errstate(over="ignore"):
        return torch.from_numpy(x.float().numpy().astype(np.float16).astype(np.float64))


def f16_trunc(x):
    """(mutation) f16 rounding toward zero"""
    x32 = x.float().numpy()
    h = x32.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x32.astype(np.float64))
    return torch.from_numpy(np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64))


def ulp16(a):
    """spacing of the f16 grid at |a| (its larger side; 2^-24 in the subnormals)"""
    with np.errstate(over="ignore", invalid="ignore"):
        h = a.abs().float().numpy().astype(np.float16)
        return torch.from_numpy(np.nextafter(h, np.float16(np.inf)).astype(np.float64) - h.astype(np.float64))


class Mut:
    """The arithmetic's switches.  exact=True: no rounding anywhere (fp64, no lo*lo dropped).  The rest are the
    plausible kernel bugs of test_conv32_emul_cpu.py's discrimination test."""

    def __init__(self, exact=False, drop_act_lo=False, drop_w_lo=False, trunc_lo=False, sample0_scale=False,
                 wz_gain=2.0, use_wscale=True, split_before_transform=False):
        self.exact = exact
        self.drop_act_lo = drop_act_lo
        self.drop_w_lo = drop_w_lo
        self.trunc_lo = trunc_lo
        self.sample0_scale = sample0_scale
        self.wz_gain = wz_gain
        self.use_wscale = use_wscale
        self.split_before_transform = split_before_transform


def split(x, mut, drop_lo):
    """hi = f16(x) (RNE), lo = f16(x - hi) (the subtraction is exact in fp32): pack_split_kernel (ops.hip),
    conv3d.hip:177-179, conv1x1.hip:69-70, split_pair (conv3d_stage.h:29)"""
    if mut.exact:
        return x, torch.zeros_like(x)
    hi = f16(x)
    lo = (f16_trunc if mut.trunc_lo else f16)(x - hi)
    return hi, (torch.zeros_like(lo) if drop_lo else lo)


def _silu(y, prec, mut):
    """prec 0: silu_f<false> (conv3d_load.h:20), y / (1 + expf(-y)) with IEEE divide; prec 1 / 3: silu_f<true> and
    the exp2 / rcp form of conv3d_stage.h:200 -- here y * sigmoid(y), the sigmoid exact and rounded.  Each fp32
    operation rounded once.  delta bounds |kernel - this| per value, as conv16_emul._silu: 2^-24 (8 + 2|y|) |v|
    covers expf or v_exp_f32 and the reciprocal / divide (1 ulp each), the rounded exponent argument and log2(e)
    (|y| 2^-24 each), 1 + e and the product (half an ulp each) on the kernel's side, and this side's roundings."""
    if mut.exact:
        return F.silu(y), torch.zeros_like(y)
    if prec == 0:
        v = r32(y / r32(1.0 + r32(torch.exp(-y))))
    else:
        v = r32(y * r32(torch.sigmoid(y)))
    return v, 2.0 ** -24 * (8.0 + 2.0 * y.abs()) * v.abs()


def _operand(s, ds, mut, drop_lo):
    """split of a scaled operand s whose kernel value may differ by ds; returns hi, lo, the bound on |a' - a|
    (a = hi + lo) and the bound on |hi' - hi|"""
    hi, lo = split(s, mut, drop_lo)
    if mut.exact:
        z = torch.zeros_like(s)
        return hi, lo, z, z
    act = ds > 0
    hflip = (f16(s + ds) - f16(s - ds)).abs()
    # |lo'|, |lo| <= |lo| + ds (hi unchanged), <= 2 (|lo| + ds) where hi can round the other way (it may cross a
    # binade); each rounds to within half an ulp of its own grid
    lo_ulp = ulp16(torch.where(hflip > 0, 2.0 * (lo.abs() + ds), lo.abs() + ds))
    da = torch.where(act, ds + lo_ulp, torch.zeros_like(s))
    return hi, lo, da, hflip


def conv32(srcs, w, b, precision, in_mode="same", aff=None, act=False, bound=None, res=None, res_mode="none",
           mut=None):
    """Emulate ddpm3d_conv3d for precision 0 (f32), 1 (f16x3 direct / 1x1 / last layer), 3 (f16x3 Winograd-D).

    srcs: one or two NCDHW fp32 tensors (the virtual concat; in_mode "planar": the two single-channel volumes)
    w, b: fp32 OIDHW weights (k = 1 or 3) and bias; aff: (A, B) [N, Cin] fp32; act: SiLU after the affine
    in_mode: "same" | "up" | "pool" | "stride2" | "planar"; res_mode: "none" | "same" | "up" | "pool"
    bound: [N, k] fp32 in_bound entries (the split modes); mut: Mut (default: the kernels' arithmetic).
    Returns a dict of NCDHW fp64 tensors: out, stored, absterms, sqterms, trabs, silu; and the scales used."""
    mut = mut or Mut()
    exact = mut.exact
    x = torch.cat([s.double() for s in srcs], dim=1)
    N, Cin = x.shape[0], x.shape[1]
    Cout, k = w.shape[0], w.shape[2]
    # ---- the input as the matrix cores see it, before scaling: v = act(fma(x, A, B)) per source voxel
    # (halo_finish / halo_fetch, conv3d_load.h:111-216; stage_write, conv3d_stage.h:196: the same value times S)
    if aff is not None and in_mode != "planar":
        A = aff[0].double().reshape(N, Cin, 1, 1, 1).expand_as(x)
        B = aff[1].double().reshape(N, Cin, 1, 1, 1).expand_as(x)
        y = x * A + B if exact else fma32(x, A, B)
    else:
        y = x
    if act:
        v, delta = _silu(y, precision, mut)
    else:
        v, delta = y, torch.zeros_like(y)
    if in_mode == "up":
        v, delta = _up(v), _up(delta)
    elif in_mode == "pool":
        # fp32 ((s00 + s01) + s10) + s11, * 1/4 (conv3d_load.h:149): three roundings of at most the window's |sum|
        s_abs = _pool(v.abs(), True)
        v = _pool(v, exact)
        delta = (_pool(delta, True) + 3 * 2.0 ** -23 * s_abs) if act else torch.zeros_like(v)
    # ---- the activation scale (act_scale_finish, conv3d_load.h:229): per sample, gain 2 on the Winograd-D form
    wz = precision in WZ_MODES
    if precision in SPLIT_MODES and not exact:
        gain = mut.wz_gain if wz else 1.0
        S = [act_scale(bound[0 if mut.sample0_scale else n].numpy(), gain) for n in range(N)]
    else:
        S = [1.0] * N
    Sv = torch.tensor(S, dtype=torch.float64).reshape(N, 1, 1, 1, 1)
    stride, pad = ((1, 2, 2) if in_mode == "stride2" else 1), k // 2
    if not wz:
        conv = lambda t, ww: F.conv3d(t, ww, stride=stride, padding=pad)
        if precision == 0:
            # fp32 operands and weights (pack_weight_kernel: a plain copy), exact products
            w64 = w.double()
            out = conv(v, w64)
            absterms = conv(v.abs(), w64.abs())
            sq = conv(v * v, w64 * w64) + out * out
            silu = conv(delta, w64.abs())
            sw = torch.ones(Cout, dtype=torch.float64)
        else:
            ahi, alo, da, hfl = _operand(v * Sv, delta * Sv, mut, mut.drop_act_lo)
            ahi, alo, da, hfl = ahi / Sv, alo / Sv, da / Sv, hfl / Sv
            whi, wlo, sw = _weights(w.double(), mut, dims=(1, 2, 3, 4))
            out = conv(ahi, whi) + conv(ahi, wlo) + conv(alo, whi)
            a, wq = ahi + alo, whi + wlo
            absterms = conv(a.abs(), wq.abs())
            sq = conv(a * a, wq * wq) + out * out
            silu = conv(da, whi.abs()) + conv(hfl, wlo.abs())
        trabs = torch.zeros_like(out)
    else:
        out, absterms, sq, silu, trabs, sw = _winograd(v, delta, Sv, w, mut)
    # ---- epilogue: acc * (wscale * 1/S) (exact: powers of two) + bias (+ residual), fp32 (conv3d_epilogue.h:474-476)
    out = out + b.double().reshape(1, Cout, 1, 1, 1)
    absterms = absterms + b.double().abs().reshape(1, Cout, 1, 1, 1)
    if res_mode != "none":
        r = res.double()
        r = {"same": lambda t: t, "up": _up, "pool": lambda t: _pool(t, exact)}[res_mode](r)
        out = out + r
        absterms = absterms + r.abs()
    stored = out if exact else r32(out)
    return dict(out=out, stored=stored, absterms=absterms, sqterms=sq, trabs=trabs, silu=silu, S=S, wscale=sw)


def _weights(wt, mut, dims):
    """per-cout scale s = 2^floor(log2(8 / max|w|)) (pack_scale_kernel over the form's taps), w * s in fp32
    (exact), split; returned unscaled (exact)"""
    Cout = wt.shape[0]
    if mut.use_wscale and not mut.exact:
        m = wt.abs().amax(dim=dims)
        sw = torch.tensor([weight_scale(np.float32(m[c].item())) for c in range(Cout)], dtype=torch.float64)
    else:
        sw = torch.ones(Cout, dtype=torch.float64)
    shape = (Cout,) + (1,) * len(dims)
    s = sw.reshape(shape)
    hi, lo = split(r32(wt * s) if not mut.exact else wt * s, mut, mut.drop_w_lo)
    return hi / s, lo / s, sw


def _winograd(v, delta, Sv, w, mut):
    """The Winograd F(2,3)-along-depth form as the algorithm: transformed planes, four (1,3,3) convolutions, the
    output transform.  Output z-pair p reads input planes 2p-1 .. 2p+2 (zero outside the volume)."""
    N, Cin, D, H, W = v.shape
    Cout = w.shape[0]
    P = (D + 1) // 2
    rr = (lambda t: t) if mut.exact else r32
    vp = F.pad(v * Sv, (0, 0, 0, 0, 1, 2 * P + 1 - D))
    dp = F.pad(delta * Sv, (0, 0, 0, 0, 1, 2 * P + 1 - D))
    d = [vp[:, :, j + 2 * torch.arange(P)] for j in range(4)]
    dd = [dp[:, :, j + 2 * torch.arange(P)] for j in range(4)]
    # input transform in stage_write (conv3d_stage.h:224-227): d0-d2, d1+d2, d2-d1, d1-d3 in fp32, then the split
    pairs, sgn = [(0, 2), (1, 2), (2, 1), (1, 3)], [-1.0, 1.0, -1.0, -1.0]
    thi, tlo, tda, thf = [], [], [], []
    for j, (p0, p1) in enumerate(pairs):
        t = rr(d[p0] + sgn[j] * d[p1])
        dt = dd[p0] + dd[p1]
        dt = dt + 2.0 ** -23 * (t.abs() + dt) * (dt > 0)
        if mut.split_before_transform:
            # (mutation) each plane split first, the transform applied to the f16 halves in f16
            h0, l0 = split(d[p0], mut, mut.drop_act_lo)
            h1, l1 = split(d[p1], mut, mut.drop_act_lo)
            hi, lo = f16(h0 + sgn[j] * h1), f16(l0 + sgn[j] * l1)
            da, hf = torch.zeros_like(t), torch.zeros_like(t)
        else:
            hi, lo, da, hf = _operand(t, dt, mut, mut.drop_act_lo)
        thi.append(hi / Sv)
        tlo.append(lo / Sv)
        tda.append(da / Sv)
        thf.append(hf / Sv)
    # weight transform wz_weight (ops.hip): U0 = g0, U1 = 0.5*((g0+g2)+g1), U2 = 0.5*((g0+g2)-g1), U3 = g2, fp32
    g = [w[:, :, z].double() for z in range(3)]
    g02 = rr(g[0] + g[2])
    U = [g[0], rr(0.5 * rr(g02 + g[1])), rr(0.5 * rr(g02 - g[1])), g[2]]
    # one scale per cout over all 36 transformed taps, then the split (pack_scale_kernel, pack_split_kernel on WzTaps)
    Ust = torch.stack(U, dim=1)                                    # [Cout, 4, Cin, 3, 3]
    Uhi, Ulo, sw = _weights(Ust, mut, dims=(1, 2, 3, 4))
    conv = lambda a, u: F.conv3d(a, u.unsqueeze(2), padding=(0, 1, 1))
    M, Ma, Mq, Ms = [], [], [], []
    for j in range(4):
        uh, ul = Uhi[:, j], Ulo[:, j]
        m = conv(thi[j], uh) + conv(thi[j], ul) + conv(tlo[j], uh)
        a, u = thi[j] + tlo[j], uh + ul
        M.append(m)
        Ma.append(conv(a.abs(), u.abs()))
        Mq.append(conv(a * a, u * u) + m * m)
        Ms.append(conv(tda[j], uh.abs()) + conv(thf[j], ul.abs()))

    def otr(X, sub):
        # output transform (conv3d_wz.h:260-261): M0 + M1 + M2, M1 - M2 - M3; interleave the pairs, crop D
        z0 = X[0] + X[1] + X[2]
        z1 = X[1] - X[2] - X[3] if sub else X[1] + X[2] + X[3]
        o = torch.stack([z0, z1], dim=3).reshape(N, Cout, 2 * P, H, W)
        return o[:, :, :D]

    return (otr(M, True), otr(Ma, False), otr(Mq, False), otr(Ms, False), otr([m.abs() for m in M], False), sw)
