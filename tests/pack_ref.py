"""
The expected bytes of every packed weight image (ddpm3d_pack_conv_weight, ddpm3d_pack_up_phase_weight), for the tests.

No weight arithmetic of its own: the taps of a form, the per-cout scale, the hi/lo split and the bf16 rounding are
the emulators' (conv32_up_emul.wz_weights / phase_sum, conv16_emul.weight_scale / Rounding, conv32_emul.r32 /
split).  What this file adds is the arrangement into the layouts of conv3d_params.h PackedImage and the zero padding:

  precision 0        fp32 [tap][ci/8][CoutPad][8]
  every other one    16-bit [tap][ci/16][hi|lo][CoutPad][16], then CoutPad fp32 output scales 1 / s
                     (f16 forms: hi, lo = the split of w * s; bf16 forms: hi = bf16(w), lo = 0, scales 1)
  the phase buffer   the precision-3 image, then the 64-tap phase image in the same 16-bit layout

with CoutPad = Cout rounded up to 32, CinPad = Cin rounded up to 16, and the taps of a form ordered

  "plain"  (dz, dy, dx) of the OIDHW weights (27, or 1);
  "wz"     (j, dy, dx) of the Winograd-along-depth transform (36): precisions 3, 4, 6;
  "up"     (phase, j, a, b) of the phase sums (64).

`weights` builds the seeded inputs of the image tests, the four special couts included, and asserts the one
condition under which a device image can be compared bit for bit (see there).
"""

import math

import numpy as np
import torch

import conv32_emul as E
import conv32_up_emul as UE
from conv16_emul import W_TARGET, Rounding, weight_scale

WZ_PRECISIONS = (3, 4, 6)
BF16_PRECISIONS = (5, 6)
# couts 1..4 of every test input: what their largest |weight| is
SPECIAL = {1: 0.0, 2: 1e-30, 3: 1e10, 4: 3.2e38}
SPECIAL_SCALE = {1: 1.0, 2: 2.0 ** 24, 3: 2.0 ** -24, 4: 1.0}
LOG2_MARGIN = 2.0 ** -10


def pads(Cout, Cin):
    return -(-Cout // 32) * 32, -(-Cin // 16) * 16


def form_of(precision):
    return "wz" if precision in WZ_PRECISIONS else "plain"


def form_taps(w, form):
    """[Cout, Cin, taps] fp64 holding the fp32 value of every tap of the form"""
    Cout, Cin = w.shape[:2]
    if form == "plain":
        return w.double().reshape(Cout, Cin, -1)
    U = UE.wz_weights(w, E.Mut())                                  # [Cout, 4, Cin, 3, 3]
    if form == "wz":
        return U.permute(0, 2, 1, 3, 4).reshape(Cout, Cin, 36)
    P = UE.phase_sum(U, E.Mut(), UE.PMut())                        # [Cout, phase, j, Cin, a, b]
    return P.permute(0, 3, 1, 2, 4, 5).reshape(Cout, Cin, 64)


def scales(taps):
    """s per cout over all taps of the form (fp64 tensor)"""
    m = taps.abs().amax(dim=(1, 2))
    return torch.tensor([weight_scale(np.float32(m[c].item())) for c in range(taps.shape[0])], dtype=torch.float64)


def _arrange(a, block):
    """[Cout, Cin, taps] -> zero padded [taps, CinPad / block, CoutPad, block]"""
    Cout, Cin, taps = a.shape
    CoutPad, CinPad = pads(Cout, Cin)
    p = np.zeros((CoutPad, CinPad, taps), dtype=a.dtype)
    p[:Cout, :Cin] = a
    return np.ascontiguousarray(p.reshape(CoutPad, CinPad // block, block, taps).transpose(3, 1, 0, 2))


def _bytes(*arrays):
    return torch.from_numpy(np.concatenate([np.frombuffer(a.tobytes(), dtype=np.uint8) for a in arrays]))


def image16(taps, bf16):
    """the 16-bit image of the taps and its scales, as bytes (uint8 tensor)"""
    Cout, Cin, _ = taps.shape
    if bf16:
        sw = torch.ones(Cout, dtype=torch.float64)
        hi = Rounding(5).r16(taps).float().bfloat16().view(torch.int16).numpy()      # exact: already bf16 values
        lo = np.zeros_like(hi)
    else:
        sw = scales(taps)
        h, l = E.split(E.r32(taps * sw.reshape(Cout, 1, 1)), E.Mut(), False)
        with np.errstate(over="ignore"):
            hi, lo = h.numpy().astype(np.float16), l.numpy().astype(np.float16)     # exact: already f16 values
    wscale = np.ones(pads(Cout, Cin)[0], dtype=np.float32)
    wscale[:Cout] = (1.0 / sw).numpy().astype(np.float32)
    return _bytes(np.stack([_arrange(hi, 16), _arrange(lo, 16)], axis=2), wscale)


def image(w, precision):
    """bytes of ddpm3d_pack_conv_weight's image of the OIDHW fp32 weights w"""
    taps = form_taps(w, form_of(precision))
    if precision == 0:
        return _bytes(_arrange(taps.numpy().astype(np.float32), 8))
    return image16(taps, precision in BF16_PRECISIONS)


def up_phase_image(w):
    """bytes of ddpm3d_pack_up_phase_weight's buffer: (front = the precision-3 image, the phase image)"""
    return image(w, 3), image16(form_taps(w, "up"), False)


def padding(Cout, Cin, taps, precision):
    """bool per byte of an image's taps (its body): True where the byte belongs to a padded cout or ci"""
    real = np.ones((Cout, Cin, taps), dtype=np.uint8)
    if precision == 0:
        elems = _arrange(real, 8)
    else:
        elems = np.stack([_arrange(real, 16)] * 2, axis=2)
    return torch.from_numpy(np.repeat(elems.reshape(-1) == 0, 4 if precision == 0 else 2))


def log2_margin(m):
    """distance of log2(fl32(W_TARGET / m)) from the nearest integer"""
    lg = math.log2(float(np.float32(W_TARGET) / np.float32(m)))
    return abs(lg - round(lg))


def weights(Cout, Cin, k, seed, forms):
    """Seeded OIDHW fp32 weights: normal draws times a per-cout power-of-ten-ish magnitude, and couts 1..4 as SPECIAL
    says (largest |weight| exactly that value; the 3.2e38 one alone in its (ci, dy, dx) column of zeros below it so
    that no transform overflows).

    Asserted, for every other cout and every form in `forms`: log2(fl32(8 / m)), m the largest |tap| of the form,
    lies at least 2^-10 from an integer, so that a last-ulp difference in a log2 cannot move its floor.  The
    special couts need no margin: their scales are set by a clamp or a branch, two and more binades away."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, k, k, k, generator=g)
    w = w * torch.exp2(8.0 * torch.rand(Cout, 1, 1, 1, 1, generator=g) - 4.0)
    for c, top in SPECIAL.items():
        flat = w[c].reshape(-1)
        at = int(flat.abs().argmax())
        if top == 0.0:
            flat.zero_()
        elif top > 1e38:
            at = 0                              # (ci 0, dz 0, dy 0, dx 0)
            w[c, 0, :, 0, 0] = 0.0
            flat[at] = top
        else:
            flat.mul_(top / float(flat[at].abs()))
            flat.clamp_(-top, top)
            flat[at] = top
        assert float(w[c].abs().max()) == float(np.float32(top))
    for form in forms:
        taps = form_taps(w, form)
        assert torch.isfinite(taps).all()
        m = taps.abs().amax(dim=(1, 2))
        sw = scales(taps)
        for c in range(Cout):
            if c in SPECIAL:
                assert sw[c].item() == SPECIAL_SCALE[c], (form, c, sw[c].item())
            else:
                assert log2_margin(m[c].item()) >= LOG2_MARGIN, (form, c, seed)
                assert 2.0 ** -24 < sw[c].item() < 2.0 ** 24
    return w


# the inputs of test_gpu_pack.py: (Cout, Cin, k) -> (seed, the forms whose scales must keep the margin).  A seed
# that misses the margin is replaced here, never worked around at run time.
CASES = {
    (5, 3, 3): (0, ("plain",)),
    (5, 3, 1): (0, ("plain",)),
    (40, 24, 3): (0, ("plain",)),
    (40, 24, 1): (0, ("plain",)),
    (128, 16, 3): (0, ("wz", "up")),
    (128, 32, 3): (0, ("wz",)),
}


def case_weights(Cout, Cin, k):
    seed, forms = CASES[(Cout, Cin, k)]
    return weights(Cout, Cin, k, seed, forms)
