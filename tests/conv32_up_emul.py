"""
CPU emulation of the phase form of an up-sampled-input conv (DDPM3D_HINT_UP_PHASE, include/ddpm3d.h): the f16x3
Winograd-D arithmetic of conv32_emul.py (precision 3) with the nearest-(1,2,2) up-sampling folded into the weights.

On the up-sampled plane the nine (dy, dx) taps of an output voxel of parity (py, px) meet 2x2 source voxels:
py = 0 reads source row i-1 at dy = 0 and row i at dy = 1, 2; py = 1 reads row i at dy = 0, 1 and row i+1 at
dy = 2; the same along x.  So each of the four phases is a conv with a 2x2 in-plane footprint on the source grid.

What rounds, and where (ops.hip wz_up_weight behind WzUpTaps, pack_scale_kernel / pack_split_kernel; conv3d_wz.h PHASE):
  * the input exactly as conv32_emul's Winograd-D form -- affine, SiLU, activation scale (gain 2), fp32 input
    transform along depth, hi/lo split -- on the SOURCE grid (each source voxel once);
  * the weights: U_j[dy][dx] as wz_weight (fp32), summed per phase over the collapsing group in fp32, added in
    (dy, dx) row-major order; ONE power-of-two scale per cout over all 64 phase taps; then the hi/lo split;
  * products hi*hi + hi*lo + lo*hi exact, sums fp64, output transform and epilogue as conv32_emul.

Returns conv32's dict (out, stored, absterms, sqterms, trabs, silu, S, wscale).  `PMut` holds the phase form's own
plausible bugs (test_conv32_up_emul_cpu.py); `mut` is conv32_emul.Mut.
"""

import numpy as np
import torch
import torch.nn.functional as F

import conv32_emul as E
from conv16_emul import _up, act_scale, fma32, weight_scale

# parity -> the taps d that meet source offset a = 0 (first 2x2 row / column) and a = 1
GROUPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}


class PMut:
    """wrong_grouping: each parity sums the other parity's tap groups; sum_after_split: the 36 taps are scaled and
    split first and the halves are summed in f16; scale36: the image is scaled over the 64 phase taps but the
    epilogue multiplies by the inverse of the 36-tap scale (the Winograd-D image's own); swap_parity: a phase's
    result lands on the other parity's voxels."""

    def __init__(self, wrong_grouping=False, sum_after_split=False, scale36=False, swap_parity=False):
        self.wrong_grouping = wrong_grouping
        self.sum_after_split = sum_after_split
        self.scale36 = scale36
        self.swap_parity = swap_parity


def wz_weights(w, mut):
    """U [Cout, 4, Cin, 3, 3]: wz_weight (ops.hip), fp32"""
    rr = (lambda t: t) if mut.exact else E.r32
    g = [w[:, :, z].double() for z in range(3)]
    g02 = rr(g[0] + g[2])
    return torch.stack([g[0], rr(0.5 * rr(g02 + g[1])), rr(0.5 * rr(g02 - g[1])), g[2]], dim=1)


def phase_sum(U, mut, pm):
    """[Cout, 4 phases, 4, Cin, 2, 2]: wz_up_weight's fp32 sums over the collapsing groups, row-major (dy, dx)"""
    rr = (lambda t: t) if mut.exact else E.r32
    groups = {0: GROUPS[1], 1: GROUPS[0]} if pm.wrong_grouping else GROUPS
    Cout, _, Cin = U.shape[:3]
    out = torch.zeros(Cout, 4, 4, Cin, 2, 2, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    s = None
                    for dy in groups[py][a]:
                        for dx in groups[px][b]:
                            u = U[:, :, :, dy, dx]
                            s = u if s is None else rr(s + u)
                    out[:, 2 * py + px, :, :, a, b] = s
    return out


def phase_weights(w, mut, pm):
    """hi, lo [Cout, 4, 4, Cin, 2, 2] (unscaled, exact) and the per-cout scale the epilogue undoes"""
    U = wz_weights(w, mut)
    dims = (1, 2, 3, 4, 5)
    if pm.sum_after_split:
        uh, ul, sw = E._weights(U, mut, dims=(1, 2, 3, 4))
        s = sw.reshape(-1, 1, 1, 1, 1)
        nr = E.Mut(exact=True)      # sums only; the halves are rounded to f16 below
        hi = E.f16(phase_sum(uh * s, nr, pm)) / s.unsqueeze(-1)
        lo = E.f16(phase_sum(ul * s, nr, pm)) / s.unsqueeze(-1)
        return hi, lo, sw
    hi, lo, sw = E._weights(phase_sum(U, mut, pm), mut, dims=dims)
    if pm.scale36 and not mut.exact:
        m36 = U.abs().amax(dim=(1, 2, 3, 4))
        s36 = torch.tensor([weight_scale(np.float32(m36[c].item())) for c in range(U.shape[0])], dtype=torch.float64)
        f = (sw / s36).reshape(-1, 1, 1, 1, 1, 1)       # scaled by sw, un-scaled by s36
        hi, lo = hi * f, lo * f
    return hi, lo, sw


def conv32_up(srcs, w, b, aff=None, act=False, bound=None, res=None, res_mode="none", mut=None, pmut=None):
    """Emulate ddpm3d_conv3d with DDPM3D_HINT_UP_PHASE: precision 3, in_mode "up"; arguments as conv32_emul.conv32
    (srcs at the SOURCE resolution D x H/2 x W/2)."""
    mut, pm = mut or E.Mut(), pmut or PMut()
    exact = mut.exact
    x = torch.cat([s.double() for s in srcs], dim=1)
    N, Cin, D, Hl, Wl = x.shape
    Cout = w.shape[0]
    if aff is not None:
        A = aff[0].double().reshape(N, Cin, 1, 1, 1).expand_as(x)
        B = aff[1].double().reshape(N, Cin, 1, 1, 1).expand_as(x)
        y = x * A + B if exact else fma32(x, A, B)
    else:
        y = x
    v, delta = E._silu(y, 3, mut) if act else (y, torch.zeros_like(y))
    S = [1.0] * N if exact else [act_scale(bound[0 if mut.sample0_scale else n].numpy(), mut.wz_gain) for n in range(N)]
    Sv = torch.tensor(S, dtype=torch.float64).reshape(N, 1, 1, 1, 1)
    # ---- the transformed planes of the source grid (conv32_emul._winograd's input side)
    P = (D + 1) // 2
    rr = (lambda t: t) if exact else E.r32
    vp = F.pad(v * Sv, (0, 0, 0, 0, 1, 2 * P + 1 - D))
    dp = F.pad(delta * Sv, (0, 0, 0, 0, 1, 2 * P + 1 - D))
    d = [vp[:, :, j + 2 * torch.arange(P)] for j in range(4)]
    dd = [dp[:, :, j + 2 * torch.arange(P)] for j in range(4)]
    pairs, sgn = [(0, 2), (1, 2), (2, 1), (1, 3)], [-1.0, 1.0, -1.0, -1.0]
    thi, tlo, tda, thf = [], [], [], []
    for j, (p0, p1) in enumerate(pairs):
        t = rr(d[p0] + sgn[j] * d[p1])
        dt = dd[p0] + dd[p1]
        dt = dt + 2.0 ** -23 * (t.abs() + dt) * (dt > 0)
        hi, lo, da, hf = E._operand(t, dt, mut, mut.drop_act_lo)
        thi.append(hi / Sv)
        tlo.append(lo / Sv)
        tda.append(da / Sv)
        thf.append(hf / Sv)
    Uhi, Ulo, sw = phase_weights(w, mut, pm)

    def pconv(a, u, py, px):
        """2x2 conv of phase (py, px): tap (a, b) reads source (y + a + py - 1, x + b + px - 1), zero outside"""
        o = F.conv3d(F.pad(a, (1, 1, 1, 1)), u.unsqueeze(2))
        return o[:, :, :, py:py + Hl, px:px + Wl]

    def full():
        return torch.zeros(N, Cout, P, 2 * Hl, 2 * Wl, dtype=torch.float64)

    M, Ma, Mq, Ms = [], [], [], []
    for j in range(4):
        m, ma, mq, ms = full(), full(), full(), full()
        for py in range(2):
            for px in range(2):
                uh, ul = Uhi[:, 2 * py + px, j], Ulo[:, 2 * py + px, j]
                pm_ = pconv(thi[j], uh, py, px) + pconv(thi[j], ul, py, px) + pconv(tlo[j], uh, py, px)
                a, u = thi[j] + tlo[j], uh + ul
                oy, ox = (1 - py, 1 - px) if pm.swap_parity else (py, px)
                m[..., oy::2, ox::2] = pm_
                ma[..., oy::2, ox::2] = pconv(a.abs(), u.abs(), py, px)
                mq[..., oy::2, ox::2] = pconv(a * a, u * u, py, px) + pm_ * pm_
                ms[..., oy::2, ox::2] = pconv(tda[j], uh.abs(), py, px) + pconv(thf[j], ul.abs(), py, px)
        M.append(m)
        Ma.append(ma)
        Mq.append(mq)
        Ms.append(ms)

    def otr(X, sub):
        z0 = X[0] + X[1] + X[2]
        z1 = X[1] - X[2] - X[3] if sub else X[1] + X[2] + X[3]
        o = torch.stack([z0, z1], dim=3).reshape(N, Cout, 2 * P, 2 * Hl, 2 * Wl)
        return o[:, :, :D]

    out, absterms, sq, silu = otr(M, True), otr(Ma, False), otr(Mq, False), otr(Ms, False)
    trabs = otr([m.abs() for m in M], False)
    out = out + b.double().reshape(1, Cout, 1, 1, 1)
    absterms = absterms + b.double().abs().reshape(1, Cout, 1, 1, 1)
    if res_mode != "none":
        r = res.double()
        r = {"same": lambda t: t, "up": _up}[res_mode](r)
        out = out + r
        absterms = absterms + r.abs()
    stored = out if exact else E.r32(out)
    return dict(out=out, stored=stored, absterms=absterms, sqterms=sq, trabs=trabs, silu=silu, S=S, wscale=sw)
