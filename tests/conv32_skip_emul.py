"""
CPU emulation of ddpm3d_conv3d_skip's fused form (conv3d_wz.h SKIP), for the tests: the tail of a ResBlock whose skip
connection is a 1x1 conv,  out = conv2(silu(A h + B)) + skip(x) + b_conv2 + b_skip,  in ONE set of fp32 accumulators.

Restated from conv32_emul's pieces:
  * conv2: the precision-3 (f16x3 Winograd-D) accumulators up to the output transform -- conv32_emul.conv32 with a zero
    bias, in units of S_h s_conv2[c] (S_h: activation scale of h, gain 2; s_conv2: the per-cout weight scale);
  * rho_c = (S_x s_skip[c]) / (S_h s_conv2[c]), a power of two: the accumulators are multiplied by it (exact), which
    brings them to the 1x1 conv's units;
  * the skip conv: the precision-1 products of conv1x1.hip on the raw x times S_x (gain 1), hi/lo split, against the
    unchanged 1x1 image, added to the same accumulators;
  * one epilogue: times 1 / (S_x s_skip[c]) (exact), plus the fp32 sum b_conv2[c] + b_skip[c].
A split launch deals chunks and x blocks to slabs of the same units and sums them: the same terms in another order.

Returns conv32_emul's record (out, stored, absterms, sqterms, trabs, silu); what is not emulated -- the order of the
fp32 accumulation, the SiLU's last ulps -- is what test_gpu_conv32.py's bars bound.
"""

import numpy as np
import torch
import torch.nn.functional as F

import conv32_emul as E
from conv16_emul import act_scale

ALT_MAX = 2.0 - 2.0 ** -12      # mantissa of a bound just below 2 (test_gpu_conv32.py)


class SkipMut:
    """exact=True: no rounding anywhere.  The rest are the plausible bugs of the fused form."""

    def __init__(self, exact=False, drop_x_lo=False, sx_gain=1.0, use_rho=True):
        self.exact = exact
        self.drop_x_lo = drop_x_lo      # x staged without its lo halves
        self.sx_gain = sx_gain          # x staged at the Winograd-D gain (2) while rho and the epilogue use gain 1
        self.use_rho = use_rho          # conv2's accumulators left in their own units


def conv32_skip(h_srcs, w2, b2, aff, bound_h, x_srcs, w1, b1, bound_x, act=True, mut=None):
    """h_srcs, x_srcs: lists of NCDHW fp32 tensors (virtual concats); w2 [Cout, Ch, 3, 3, 3], w1 [Cout, Cx, 1, 1, 1];
    aff = (A, B) of h; bound_h / bound_x: [N, k] in_bound entries."""
    mut = mut or SkipMut()
    N, Cout = h_srcs[0].shape[0], w2.shape[0]
    zero = torch.zeros(Cout)
    e2 = E.conv32(h_srcs, w2, zero, 3, aff=aff, act=act, bound=bound_h, mut=E.Mut(exact=mut.exact))
    e1 = E.conv32(x_srcs, w1, zero, 1, bound=bound_x, mut=E.Mut(exact=mut.exact, drop_act_lo=mut.drop_x_lo))
    col = lambda t: t.double().reshape(1, Cout, 1, 1, 1)
    bias = b2.double() + b1.double()
    if mut.exact:
        out = e2["out"] + e1["out"] + col(bias)
    else:
        bias = E.r32(bias)                                             # one fp32 add
        Sh = torch.tensor(e2["S"], dtype=torch.float64).reshape(N, 1, 1, 1, 1)
        Sx = torch.tensor(e1["S"], dtype=torch.float64).reshape(N, 1, 1, 1, 1)
        Sx_staged = torch.tensor([act_scale(bound_x[n].numpy(), mut.sx_gain) for n in range(N)],
                                 dtype=torch.float64).reshape(N, 1, 1, 1, 1)
        u2, u1 = Sh * col(e2["wscale"]), Sx * col(e1["wscale"])       # the accumulators' units
        rho = u1 / u2 if mut.use_rho else torch.ones_like(u1 / u2)
        acc = (e2["out"] * u2) * rho + e1["out"] * (Sx_staged * col(e1["wscale"]))
        out = acc / u1 + col(bias)
    return dict(out=out, stored=out if mut.exact else E.r32(out),
                absterms=e2["absterms"] + e1["absterms"] + col(bias).abs(),
                sqterms=e2["sqterms"] + e1["sqterms"], trabs=e2["trabs"], silu=e2["silu"] + e1["silu"],
                S=(e2["S"], e1["S"]), wscale=(e2["wscale"], e1["wscale"]), parts=(e2, e1))


def composed(em, b2, b1):
    """The two shipped launches, from the fused record's own pieces (the same products): the 1x1 conv (precision 1)
    with its bias into out, then conv2 (precision 3) with its bias and that fp32 tensor as its same-shape residual --
    conv32_emul.conv32's epilogue applied to em["parts"].  Returns (record of the 1x1 launch, record of conv2's)."""
    e2, e1 = em["parts"]
    col = lambda t: t.double().reshape(1, -1, 1, 1, 1)
    c1 = dict(e1)
    c1["out"] = e1["out"] + col(b1)
    c1["absterms"] = e1["absterms"] + col(b1).abs()
    c1["stored"] = E.r32(c1["out"])
    c2 = dict(e2)
    c2["out"] = e2["out"] + col(b2) + c1["stored"]
    c2["absterms"] = e2["absterms"] + col(b2).abs() + c1["stored"].abs()
    c2["stored"] = E.r32(c2["out"])
    return c1, c2


def skip_inputs(N=1, D=5, H=8, W=10, Ch=128, Cx=(32,), Cout=128, mags=((1.0, 1.0),), alt_max_x=False, seed=0):
    """CPU tensors of a case.  mags: per sample (magnitude of h, magnitude of x); alt_max_x: |x| = ALT_MAX everywhere,
    the sign random.  Bounds are the true maxima of silu(A h + B) and of x."""
    g = np.random.default_rng(3000 + seed)
    rn = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    hm = torch.tensor([m[0] for m in mags], dtype=torch.float32).reshape(N, 1)
    xm = torch.tensor([m[1] for m in mags], dtype=torch.float32).reshape(N, 1, 1, 1, 1)
    h = rn(N, Ch, D, H, W)
    aff = ((1.0 + 0.1 * rn(N, Ch)) * hm, (0.1 * rn(N, Ch)) * hm)
    xs = []
    for c in Cx:
        x = rn(N, c, D, H, W)
        xs.append((torch.sign(x) * ALT_MAX if alt_max_x else x * xm).float().contiguous())
    w2 = rn(Cout, Ch, 3, 3, 3) * 0.05
    w1 = rn(Cout, sum(Cx), 1, 1, 1) * 0.1
    b2, b1 = rn(Cout) * 0.01, rn(Cout) * 0.01
    hin = F.silu(h * aff[0][:, :, None, None, None] + aff[1][:, :, None, None, None])
    bound_h = hin.abs().reshape(N, -1).amax(1, keepdim=True).float().contiguous()
    bound_x = torch.cat(xs, 1).abs().reshape(N, -1).amax(1, keepdim=True).float().contiguous()
    return dict(h=[h], w2=w2, b2=b2, aff=aff, bound_h=bound_h, xs=xs, w1=w1, b1=b1, bound_x=bound_x)


def emulate(t, **mut):
    return conv32_skip(t["h"], t["w2"], t["b2"], t["aff"], t["bound_h"], t["xs"], t["w1"], t["b1"], t["bound_x"],
                       mut=SkipMut(**mut))
