"""
The GroupNorm statistics chain at the kernel, against gn_ref.py's fp64 reference:

  (a) ddpm3d_gn_finalize on synthetic statistics rows (no conv is launched): A, B per element within
      gn_ref.finalize_bars, entry 1 of the bound bitwise, entry 0 within one ulp, repeatable, samples independent --
      at the smallest shapes that cross each branch of gn_finalize_kernel and its launcher: the 256 / 1024-thread
      switch (items = rows x C / groups = 2047, 2048, 2049), the load loop's one-pass edge (8191, 8192, 8196, 8193
      at an odd group width) and a ragged fourth pass (24580), rows0 != rows1 across a concat in both orders,
      groups 1 / 2 / 32 / C with a group wider than the workgroup, FiLM rows with padding at offsets 0 / 2C / 7, two
      eps, a mean of 1e3 standard deviations, constant / all-zero / NaN rows, the bounds-only and the no-bound forms;
  (b) ddpm3d_gn_stats against fp64 sums of the fp32 values, voxels around its 256-voxel row and C up to a second
      pass of the channel-quad loop;
  (c) the bound through every writer of statistics rows (conv3d_epilogue.h: the lean, wide, scalar and general
      epilogue sites; conv3d.hip: the two split-K reduce kernels) on one hot voxel per (sample, group) over a flat
      background of 1e-3 of it, and over none -- where the pivoted fp32 sums of GnAcc lose most -- against the
      derived slack gn_ref.delta(n), and then through the consumers that pick their activation scale from it.
      (Measured on an MI355X, 1 - bound / max|x|: at most 6.2e-5 on the 64-value lanes over an empty background,
      delta(64) = 4.0e-4; DESIGN.md section 2 has the table.)

test_gn_ref_cpu.py shows per case of (a) that each plausible kernel bug (gn_ref.Mut) moves A, B or the bound by at
least 10x the bar the case is held to.
"""

import functools
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_ref as R

pytestmark = pytest.mark.gpu

N = 3
EINVAL = -1


@pytest.fixture(scope="module")
def hc():
    import hipcall
    return hipcall


# --------------------------------------------------------------------------- (a) finalize on synthetic rows
@dataclass(frozen=True)
class Case:
    name: str
    C0: int
    rows0: int
    C1: int = 0
    rows1: int = 0
    groups: int = 32
    film: bool = False
    film_off: int = 0          # (film_stride = film_off + 2 C + 5: padded rows)
    eps: float = 1e-5
    data: str = "gauss"        # gauss | bigmean | const | zero | nan
    gamma: bool = True         # False: the bounds-only form
    bound: bool = True         # False: bound NULL

    @property
    def C(self):
        return self.C0 + self.C1

    @property
    def cg(self):
        return self.C // self.groups

    @property
    def items(self):           # what the launcher sizes the workgroup by
        return max(self.rows0, self.rows1) * self.cg


CASES = [
    # items = rows x C / groups across the thread-count switch and the one-pass edge
    Case("items_1", 32, 1),
    Case("items_6_film", 64, 3, film=True),
    Case("items_2047", 32, 2047),
    Case("items_2048_film_off_2C", 64, 1024, film=True, film_off=128),
    Case("items_2049", 96, 683),
    Case("items_8191", 32, 8191, eps=1e-3),
    Case("items_8192", 64, 4096),
    Case("items_8196_film_off_7", 128, 2049, film=True, film_off=7),
    Case("items_8193_c96", 96, 2731),
    Case("items_24580_film_off_2C", 80, 6145, groups=20, film=True, film_off=160),
    # concat
    Case("cat_64_64", 64, 7, 64, 7),
    Case("cat_96_32_film", 96, 4, 32, 9, film=True, film_off=7, eps=1e-3),
    Case("cat_rows_3_2048_film", 64, 3, 64, 2048, film=True),
    Case("cat_rows_2048_3", 64, 2048, 64, 3),
    # groups
    Case("groups_1_c1280_t1024_film", 1280, 2, groups=1, film=True, film_off=7),
    Case("groups_1_c1280_t256", 1280, 1, groups=1),
    Case("groups_2", 64, 5, groups=2),
    Case("groups_C_film", 64, 5, groups=64, film=True, film_off=128),
    # data
    Case("bigmean", 64, 6, data="bigmean"),
    Case("const", 64, 6, data="const"),
    Case("zero_film", 64, 6, data="zero", film=True, film_off=7),
    Case("nan_row", 64, 6, data="nan"),
    # forms
    Case("bounds_only_cat_96_32", 96, 4, 32, 9, gamma=False),
    Case("bounds_only_cat_rows_3_2048", 64, 3, 64, 2048, gamma=False),
    Case("no_bound", 64, 3, bound=False),
]
NAN_AT = (1, 3)      # (sample, group) of the "nan" case's NaN row


@functools.lru_cache(maxsize=None)
def inputs(name):
    """a case's statistics, parameters, fp64 reference and bars: computed once, shared, never modified"""
    c = next(k for k in CASES if k.name == name)
    g = np.random.default_rng(zlib.crc32(name.encode()))
    V = 2 * max(c.rows0, c.rows1) + 3                      # voxels per channel = `count`
    mag = np.array([1.0, 30.0, 0.01], dtype=np.float32).reshape(N, 1, 1)
    st = []
    for Ci, rows in ((c.C0, c.rows0), (c.C1, c.rows1)):
        if Ci == 0:
            st.append(None)
            continue
        x = g.standard_normal((N, Ci, V)).astype(np.float32)
        if c.data == "bigmean":
            x = (x + 1e3).astype(np.float32)
        elif c.data == "const":
            x = np.full_like(x, 2.5)
        elif c.data == "zero":
            x = np.zeros_like(x)
        else:
            x = ((x + 0.3) * mag).astype(np.float32)
        s = R.make_stats(x, R.partition(g, V, rows))
        if c.data == "nan":
            s[NAN_AT[0], NAN_AT[1] * (c.C // c.groups), rows // 2, :] = np.nan
        st.append(s)
    gamma = (1 + 0.1 * g.standard_normal(c.C)).astype(np.float32)
    beta = (0.1 * g.standard_normal(c.C)).astype(np.float32)
    stride = c.film_off + 2 * c.C + 5
    film = (0.2 * g.standard_normal((N, stride))).astype(np.float32) if c.film else None
    args = (st[0], st[1], float(V), c.eps, gamma if c.gamma else None, beta if c.gamma else None, film,
            stride if c.film else 0, c.film_off if c.film else 0, c.groups)
    ref = R.finalize_ref(*args)
    bars = R.finalize_bars(*args) if c.gamma else (None, None)
    for a in (st[0], st[1], gamma, beta, film, ref["xmax"], ref["bound0"], ref["A"], ref["B"], *bars):
        if a is not None:
            a.setflags(write=False)
    return dict(case=c, st=st, count=float(V), gamma=gamma, beta=beta, film=film, stride=stride, args=args, ref=ref,
                barA=bars[0], barB=bars[1])


def bound_bars(t):
    """what the GPU test allows the two bound entries to differ from the fp64 reference by: entry 1 is held
    bitwise (one ulp here), entry 0 to one ulp of fmaf(max|A|, xmax, max|B|) on top of A's and B's own bars"""
    c, ref = t["case"], t["ref"]
    b1 = 2.0 ** -23 * ref["xmax"]
    if not c.gamma:
        return b1, b1
    G = c.groups
    with np.errstate(invalid="ignore"):
        da = np.fmax.reduce(t["barA"].reshape(N, G, -1), axis=2, initial=0.0)
        db = np.fmax.reduce(t["barB"].reshape(N, G, -1), axis=2, initial=0.0)
    return 2.0 ** -23 * ref["bound0"] + da * ref["xmax"] + db, b1


def _launch(hc, t, st, poison):
    c = t["case"]
    cu = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    A, B, bound = hc.gn_finalize([cu(s) for s in st if s is not None], t["count"], cu(t["gamma"]) if c.gamma else None,
                                 cu(t["beta"]) if c.gamma else None, film=cu(t["film"]),
                                 film_stride=t["stride"] if c.film else 0, film_off=c.film_off if c.film else 0,
                                 groups=c.groups, with_bound=True, eps=c.eps, null_bound=not c.bound, poison=poison)
    return A.cpu().numpy(), B.cpu().numpy(), bound.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_finalize_against_fp64(hc, name):
    t = inputs(name)
    c, ref = t["case"], t["ref"]
    A, B, bound = _launch(hc, t, t["st"], float("nan"))
    A2, B2, bound2 = _launch(hc, t, t["st"], -7.25)
    G, cg = c.groups, c.cg
    if c.gamma:
        # per element, within the bars; NaN exactly where the reference is NaN
        for got, want, bar, what in ((A, ref["A"], t["barA"], "A"), (B, ref["B"], t["barB"], "B")):
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), what
            ratio = np.abs(got.astype(np.float64) - want)[~nan] / bar[~nan]
            print("%s %s: worst error / bar = %.3g (bar / |value| up to %.3g)" %
                  (name, what, ratio.max(), (bar[~nan] / np.maximum(np.abs(want[~nan]), 1e-300)).max()))
            assert (ratio <= 1.0).all(), (what, float(ratio.max()))
        # the same bits into differently poisoned buffers
        assert np.array_equal(_bits(A), _bits(A2)) and np.array_equal(_bits(B), _bits(B2))
    else:
        # bounds only: A and B are not touched
        assert np.isnan(A).all() and np.isnan(B).all() and (A2 == -7.25).all() and (B2 == -7.25).all()
    if c.bound:
        assert np.array_equal(_bits(bound), _bits(bound2))
        # entry 1: sqrtf((float) largest row sum of squares), both sides round once each
        rows_max = np.empty((N, G))
        for n in range(N):
            for g in range(G):
                src, cs = (0, g * cg) if g * cg < c.C0 else (1, g * cg - c.C0)
                rows_max[n, g] = np.fmax.reduce(t["st"][src][n, cs:cs + cg, :, 1].reshape(-1), initial=0.0)
        want1 = np.sqrt(rows_max.astype(np.float32))
        assert want1.dtype == np.float32
        assert np.array_equal(_bits(bound[..., 1]), _bits(want1))
        if c.gamma:
            # entry 0: within one ulp of fmaf(max|A_got|, xmax, max|B_got|) (NaNs ignored, like fmaxf)
            amax = np.fmax.reduce(np.abs(A.astype(np.float64)).reshape(N, G, cg), axis=2, initial=0.0)
            bmax = np.fmax.reduce(np.abs(B.astype(np.float64)).reshape(N, G, cg), axis=2, initial=0.0)
            want0 = amax * want1.astype(np.float64) + bmax
            assert (np.abs(bound[..., 0].astype(np.float64) - want0) <= 2.0 ** -23 * want0 + R.TINY32).all()
        else:
            assert np.array_equal(_bits(bound[..., 0]), _bits(want1))
    else:
        assert np.isnan(bound).all() and (bound2 == -7.25).all()        # our own buffer: never passed

    # ---- the degenerate inputs' own statements
    if c.gamma and c.data in ("const", "zero"):
        rs = 1.0 / np.sqrt(float(np.float32(c.eps)))
        sc = 1.0 + R._film_rows(t["film"], t["stride"], c.film_off, N, c.C, R.Mut())[0] if c.film else 1.0
        assert (np.abs(A - t["gamma"][None, :].astype(np.float64) * rs * sc) <= t["barA"]).all()   # variance clamps at 0
    if c.data == "zero":
        assert (bound[..., 1] == 0).all()
        assert np.array_equal(bound[..., 0], np.abs(B).reshape(N, G, cg).max(axis=2))
    if c.data == "nan":
        nanA = np.isnan(A).reshape(N, G, cg)
        want = np.zeros((N, G, cg), dtype=bool)
        want[NAN_AT] = True
        assert np.array_equal(nanA, want) and np.array_equal(np.isnan(B).reshape(N, G, cg), want)

    # ---- one sample's rows change: the other samples' groups keep their bits
    st2 = [None if s is None else s.copy() for s in t["st"]]
    for s in st2:
        if s is not None:
            s[1] *= 1.5
            s[1, :, :, 1] += 0.25
    A3, B3, bound3 = _launch(hc, t, st2, float("nan"))
    keep = [0, 2]
    assert np.array_equal(_bits(A3[keep]), _bits(A[keep])) and np.array_equal(_bits(B3[keep]), _bits(B[keep]))
    assert np.array_equal(_bits(bound3[keep]), _bits(bound[keep]))
    if c.bound:
        assert not np.array_equal(_bits(bound3[1]), _bits(bound[1]))
    else:
        assert not np.array_equal(_bits(A3[1]), _bits(A[1]))


@pytest.mark.parametrize("poison", [float("nan"), -7.25])
def test_finalize_refuses_a_straddling_group(hc, poison):
    """C0 = 32, C1 = 64, 32 groups of 3: group 10 would span both tensors -- DDPM3D_EINVAL, nothing written"""
    g = np.random.default_rng(5)
    st0 = torch.from_numpy(g.standard_normal((N, 32, 4, 2))).abs().cuda()
    st1 = torch.from_numpy(g.standard_normal((N, 64, 4, 2))).abs().cuda()
    gamma, beta = torch.ones(96).cuda(), torch.zeros(96).cuda()
    A, B, bound = hc.gn_finalize([st0, st1], 16.0, gamma, beta, with_bound=True, poison=poison, expect_rc=EINVAL)
    for buf in (A, B, bound):
        b = buf.cpu().numpy()
        assert np.isnan(b).all() if poison != poison else (b == poison).all()


# --------------------------------------------------------------------------- (b) ddpm3d_gn_stats
@pytest.mark.parametrize("C", [4, 36, 96, 1028])
@pytest.mark.parametrize("vox,mean", [(1, 0.0), (255, 0.0), (256, 1e4), (257, 0.0), (1000, 1e4), (1000, 0.0)])
def test_gn_stats_against_fp64(hc, vox, mean, C):
    """fp64 sums of the fp32 values (every product x * x is exact in fp64, and the kernel's fma keeps it so): the
    only difference is the kernel's order of at most `vox` fp64 additions per row, within vox 2^-53 sum|terms|;
    a sample's rows do not depend on its neighbours in the batch"""
    import guided_diffusion._hip as H
    g = np.random.default_rng(vox * 7 + C)
    x = (g.standard_normal((N, vox, C)) * np.array([1.0, 50.0, 1e-2]).reshape(N, 1, 1) + mean).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    st = hc.gn_stats(xd).cpu().numpy()
    rows = H.load().ddpm3d_gn_stats_rows(vox)
    assert rows == -(-vox // 256) and st.shape == (N, C, rows, 2)
    xl = np.moveaxis(x, 2, 1).astype(np.longdouble)                         # [N][C][vox]
    worst = 0.0
    for r in range(rows):
        seg = xl[:, :, r * 256:(r + 1) * 256]
        for j, terms in enumerate((seg, seg * seg)):
            want = terms.sum(axis=2)
            bar = (vox * R.U64 * np.abs(terms).sum(axis=2)).astype(np.float64)
            err = np.abs(st[:, :, r, j].astype(np.longdouble) - want).astype(np.float64)
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
            assert (err <= bar).all(), (r, j, float((err / np.maximum(bar, 1e-300)).max()))
    print("gn_stats vox=%d C=%d mean=%g: worst error / bar = %.3g" % (vox, C, mean, worst))
    for n in range(N):
        one = hc.gn_stats(xd[n:n + 1].contiguous()).cpu().numpy()
        assert np.array_equal(one[0].view(np.uint64), st[n].view(np.uint64))


# --------------------------------------------------------------------------- (c) the bound through its producers
# The writers of statistics rows at this commit, and the conv that routes to each.  n_lane = the most values one
# GnAcc takes there (conv3d_epilogue.h / conv3d.hip), which is what delta() is evaluated at:
#   lean    conv_epilogue_lean (one-MFMA Winograd-D forms, full tiles): ga[i] takes MT * 4 = 16
#   wide    conv_epilogue's WIDE form (one-MFMA direct kernels, full tiles): 16
#   scalar  conv_epilogue's four-byte fast path (exact and f16x3 direct kernels, full tiles): MT * 16 = 64
#   general conv_epilogue's bounds-checked tail (ragged tiles): at most 64
#   reduce_v4   conv_splitk_reduce_v4_kernel<RV> (Cout % 4 == 0): RV / 4
#   reduce      conv_splitk_reduce_kernel (any Cout): reduce_vox
# All take the voxel the lane meets first as the pivot: tile rows 0..7 of the first MFMA block (the corner of a
# tile and its x neighbours), the first voxel(s) of a reduce row.
DHW = (5, 9, 10)       # 8x8x2 tiles (Winograd-D: 8x8x2 as well): ragged in z, y and x; 450 voxels: a ragged reduce row
POSITIONS = [(z, y, x) for z in (0, 1, 3, 4) for y in (0, 3, 4, 7, 8) for x in (0, 1, 3, 4, 5, 7, 8, 9)]
FULL_TILE = lambda p: p[0] < 4 and p[1] < 8 and p[2] < 8      # inside a tile that lies inside the volume
WRITERS = {
    # name: (precision, ksize, C, groups, forced split, family, positions, lanes of a row)
    "lean": (4, 3, 128, 32, 1, "conv3d_p4_k3_wn4_t8", [p for p in POSITIONS if FULL_TILE(p)], 16),
    "wide": (2, 1, 128, 32, 1, "conv3d_p2_k1_wn4_t8", [p for p in POSITIONS if FULL_TILE(p)], 16),
    "scalar": (0, 1, 128, 32, 1, "conv3d_p0_k1_wn4_t8", [p for p in POSITIONS if FULL_TILE(p)], 64),
    "general": (0, 1, 128, 32, 1, "conv3d_p0_k1_wn4_t8", [p for p in POSITIONS if not FULL_TILE(p)], 64),
    "reduce_v4": (0, 1, 128, 32, 2, "conv3d_p0_k1_wn4_t8", POSITIONS, None),
    # (a conv's Cin is a multiple of 16: 80 input channels, of which the first 66 are copied)
    "reduce": (0, 1, 66, 33, 2, "conv3d_p0_k1_wn4_t8", POSITIONS, None),
}
CIN = {66: 80}
MAGS = (1e-3, 1e3)
# the background: 1e-3 of the hot voxel, and none at all -- a row of 128 voxels at 1e-3 adds 6e-5 to the square root
# and hides a shortfall of 1e-5; over an empty background every rounding of the pivoted sums shows
BACKGROUNDS = (1e-3, 0.0)


def hot_volume(C, groups, positions, rep, bg):
    """[2][Cin][D][H][W] fp32: per (sample, group) one hot voxel (a full fp32 mantissa, either sign) in one
    channel, background `bg` of it (flat to +-25 %), sample magnitudes 1e-3 and 1e3; the hot voxel's position
    walks through `positions` with the group, the sample and `rep`.  Channels from C on are background only."""
    g = np.random.default_rng(100 + rep)
    cg = C // groups
    D, H, W = DHW
    x = (bg * g.uniform(0.75, 1.25, (2, CIN.get(C, C), D, H, W))).astype(np.float32)
    for n in range(2):
        x[n] *= MAGS[n]
        for gr in range(groups):
            hot = MAGS[n] * g.uniform(1.0, 2.0) * (-1.0) ** gr
            x[n, gr * cg:(gr + 1) * cg] = bg * abs(hot) * (1.0 + 0.25 * g.uniform(-1, 1, (cg, D, H, W)))
            z, y, xx = positions[(gr + groups * rep + 7 * n) % len(positions)]
            x[n, gr * cg + (gr + rep) % cg, z, y, xx] = hot
    return torch.from_numpy(x)


@pytest.fixture(scope="module")
def consumers():
    """weights of the two consumers and nothing else (the fp64 convs are per input)"""
    g = np.random.default_rng(77)
    mk = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    return {C: dict(w1=mk(128, Cw, 1, 1, 1) * 0.05, b1=mk(128), w3=mk(128, Cw, 3, 3, 3) * 0.03, b3=mk(128))
            for C, Cw in ((128, 128), (66, 64))}     # (a conv's Cin is a multiple of 16: of 66 channels, the first 64)


@pytest.mark.parametrize("bg", BACKGROUNDS)
@pytest.mark.parametrize("writer", list(WRITERS))
def test_bound_through_every_statistics_writer(hc, consumers, writer, bg):
    import guided_diffusion._hip as H
    from test_gpu_range import chan_err
    prec, k, C, groups, split, family, positions, n_lane = WRITERS[writer]
    cg = C // groups
    D, Hh, W = DHW
    w = torch.zeros(C, CIN.get(C, C), k, k, k)
    for ch in range(C):
        w[ch, ch, k // 2, k // 2, k // 2] = 1.0          # identity 1x1 / centre-tap delta: the output is the input
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(1)), torch.full((C,), 0.05)
    reps = -(-len(positions) // groups) + 1               # every position is hot in some group, and once more
    worst = -1.0
    for rep in range(reps):
        x = hot_volume(C, groups, positions, rep, bg)
        out, stats, rows = hc.conv3d([hc.to_ndhwc(x).cuda()], w.cuda(), torch.zeros(C).cuda(), DHW, precision=prec,
                                     hint=split << H.HINT_SPLITK_SHIFT)
        assert hc.LAST_PLAN["family"] == family and hc.LAST_PLAN["split"] == split, hc.LAST_PLAN
        if split > 1:
            rv = next(r for r in (4, 8, 16) if -(-D * Hh * W // r) == rows)
            n_lane = rv // 4 if C % 4 == 0 else rv
        d = R.delta(n_lane)
        # delta plus the scale's own rounding stays inside the factor of two between 2^15 and f16's largest value:
        #     2^15 (1 + 2^-11) / (1 - delta) <= 65504
        assert R.headroom_ok(d) and 2.0 ** 15 * (1 + 2.0 ** -11) / (1 - d) <= 65504.0
        A, B, bound = hc.gn_finalize([stats], D * Hh * W, gamma.cuda(), beta.cuda(), groups=groups, with_bound=True)
        st = stats.cpu().numpy()
        assert np.isfinite(st).all() and (st[..., 1] >= 0).all()
        xo = hc.to_ncdhw(out.cpu()).double().numpy()                       # what the writer saw
        if prec == 0:
            assert np.array_equal(xo, x[:, :C].double().numpy())           # the exact mode copies
        Ad, Bd, bd = A.cpu().double().numpy(), B.cpu().double().numpy(), bound.cpu().double().numpy()
        xg = xo.reshape(2, groups, cg, -1)
        xmax = np.abs(xg).max(axis=(2, 3))
        ymax = np.abs(xg * Ad.reshape(2, groups, cg, 1) + Bd.reshape(2, groups, cg, 1)).max(axis=(2, 3))
        tot2 = st[..., 1].reshape(2, groups, -1).sum(axis=2)
        total = np.sqrt(tot2)
        # the rows themselves: a group's sums against the fp64 sums of what was stored, within the lanes' slack
        # (sum x = n p + s1 carries one recursive fp32 sum of |x - p| <= |x| + |p|: gamma_n (sum|x| + n max|x|))
        sq = (xg * xg).sum(axis=(2, 3))
        assert (np.abs(tot2 - sq) <= (R.sum2_slack(n_lane) + 64 * R.U64) * sq).all()     # (64 u64: these fp64 sums' own)
        lin = np.abs(st[..., 0].reshape(2, groups, -1).sum(axis=2) - xg.sum(axis=(2, 3)))
        assert (lin <= 2 * (n_lane + 2) * R.U32 * (np.abs(xg).sum(axis=(2, 3)) + cg * D * Hh * W * xmax)).all()
        short = float((1.0 - bd[..., 1] / xmax).max())
        worst = max(worst, short)
        print("%s bg %g rep %d: lanes of %d, delta %.3g, largest shortfall of entry 1: %.3g" % (writer, bg, rep, n_lane, d, short))
        assert (bd[..., 1] >= xmax * (1 - d)).all()
        assert (bd[..., 1] <= total * (1 + 2.0 ** -23)).all()
        assert (bd[..., 0] >= ymax * (1 - d)).all()
        if rep:
            continue
        # ---- the consumers: an f16x3 conv on the raw tensor (entry 1) and a Winograd-D conv behind the GroupNorm
        # (entry 0), each with one bound per group; bars of test_gpu_range.py (1x1 skip conv: 2e-6; Winograd-D
        # behind an affine with SiLU: 8e-6)
        cw = consumers[C]
        Cw = cw["w3"].shape[1]
        gw = Cw // cg
        src = out if Cw == C else out[..., :Cw].contiguous()
        o1, _, _ = hc.conv3d([src], cw["w1"].cuda(), cw["b1"].cuda(), DHW, precision=1, want_stats=False,
                             bound=bound[:, :gw, 1].contiguous())
        assert torch.isfinite(o1).all()
        ref1 = F.conv3d(torch.from_numpy(xo[:, :Cw]), cw["w1"].double(), cw["b1"].double())
        e1 = chan_err(hc.to_ncdhw(o1.cpu()), ref1)
        o3, _, _ = hc.conv3d([src], cw["w3"].cuda(), cw["b3"].cuda(), DHW, precision=3,
                             aff=(A[:, :Cw].contiguous(), B[:, :Cw].contiguous()), act=H.ACT_SILU, want_stats=False,
                             bound=bound[:, :gw, 0].contiguous())
        assert torch.isfinite(o3).all()
        xin = F.silu(torch.from_numpy(xo[:, :Cw] * Ad[:, :Cw, None, None, None] + Bd[:, :Cw, None, None, None]))
        ref3 = F.conv3d(xin, cw["w3"].double(), cw["b3"].double(), padding=1)
        e3 = chan_err(hc.to_ncdhw(o3.cpu()), ref3)
        print("%s consumers: f16x3 1x1 %.3g (bar 2e-6), Winograd-D %.3g (bar 8e-6)" % (writer, e1, e3))
        assert e1 < 2e-6 and e3 < 8e-6, (e1, e3)
    print("%s bg %g: largest shortfall over %d launches %.3g (delta %.3g)" % (writer, bg, reps, worst, d))
