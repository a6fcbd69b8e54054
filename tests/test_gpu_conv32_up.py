"""
The phase form of the up-sampled-input f16x3 Winograd-D conv (DDPM3D_HINT_UP_PHASE: four 2x2 phase convs on the
low-resolution source, 16 taps per chunk instead of 36) against the emulation of ITS arithmetic
(conv32_up_emul.py), element by element, with the model of test_gpu_conv32.py:

  |got - emul| <= E_acc + silu,   E_acc = 8 u sqrt(m sqterms / 3) + 2u (trabs + |out|),
  m = 3 (4 CinPad) + S + 8 (+ 16 when split)

-- an accumulator of the phase form takes 2 x 2 taps per input channel where the 36-tap form takes 9.  And, since
the form regroups the same products ("results stay what they were"): the result also lies within the bound
test_gpu_conv32.py holds the 36-tap kernel to (its `elem_bound`, m = 3 (9 CinPad) + ...) around the 36-tap form's
own emulation (conv32_emul.conv32).  Every case runs twice (bitwise equal); statistics against the fp64 sums of the
emulation; statistics rows and workspace are what ddpm3d_conv_stats_rows / _workspace_bytes report for the shape.
A case is known to have taken the phase form by its bits: they differ from the unhinted call's (the phase weights
are rounded after the sum), while a shape whose low-resolution grid does not tile must equal it bit for bit.

test_up_phase_error_against_fp64_within_twice_f32: the existing formula on the same cases,
max|f16x3 - ref| <= 2 max|f32 - ref| + 4u max|ref| per (sample, cout).

Shapes: the output grid D x H x W; the phase form tiles the SOURCE grid D x H/2 x W/2 (8x4x4 tiles where
H/2 % 8 == 0 and D % 4 == 0, else 8x8x2, 4x4x8 below 8x8) and is taken where 4 x those tiles = the output
grid's 8x8x2 tile count (conv3d_params.h ddpm3d_up_phase_geom).
"""

import dataclasses
import functools

import pytest
import torch

import conv32_emul as E
import conv32_up_emul as UE
import test_gpu_conv32 as G

pytestmark = pytest.mark.gpu

U = G.U
FAM = "conv3d_p3_k3_wn4_t8"
PHASE, PLAIN = "conv3d_wz_kernel<3,4,%s>", "conv3d_wz_kernel<0,4,%s>"     # <mode: 3 phase / 0 plain f16x3, issue order, TX, TY>
# (inst: the phase instance on the SOURCE grid's tile form; wz: the plain instance's tile, which the unhinted call runs)
T882 = dict(D=5, H=16, W=28, inst=PHASE % "8,8", wz="8,8")      # source 5 x 8 x 14: 8x8x2 tiles, odd D, ragged W
T844 = dict(D=8, H=16, W=28, inst=PHASE % "8,4", wz="8,4")      # source 8 x 8 x 14: 8x4x4 tiles, ragged W
T448 = dict(D=7, H=8, W=12, inst=PHASE % "4,4", wz="8,8")       # source 7 x 4 x 6: 4x4x8 tiles, odd D, ragged W
D64 = dict(D=64, wz="8,4")        # the published levels: depth 64, H % 8 == 0


def _case(name, **kw):
    return G.Case("up_" + name, 3, FAM, in_mode="up", **kw)


CASES = []
for geo, g in ((T882, "t8x8x2"), (T844, "t8x4x4"), (T448, "t4x4x8")):
    for sp, sk in ((dict(), ""), (G.FS, "_split")):
        CASES += [_case("%s%s" % (g, sk), **geo, **sp),
                  _case("%s_resid%s" % (g, sk), res_mode="same", **geo, **sp),
                  _case("%s_resid_up%s" % (g, sk), res_mode="up", **geo, **sp)]
CASES += [
    _case("d1", D=1, H=16, W=16, inst=PHASE % "8,8", res_mode="same"),
    _case("concat_resid_up", C=(16, 16), res_mode="up", **T882),
    # (64 input channels: the rule splits them in two)
    _case("concat_rule_split_resid_up", C=(32, 32), res_mode="up", expect_split=True, **T844),
    _case("two_cout_blocks", Cout=256, **T882),
    _case("two_samples_1e6", N=2, mags=(1e-6, 1.0), **T882),
    _case("small_cout", small_cout=True, **T844),
    _case("alternating_max", alt_max=True, **G.NOIN, **T844),
    _case("alternating_max_t4", alt_max=True, **G.NOIN, **T448),
    # conv1 of the published network's four up-ResBlocks at 1 x 64^3 (rule's split: 8, 2, none, none)
    _case("published_384_64x8x8", H=8, W=8, inst=PHASE % "4,4", C=(384,), Cout=384, expect_split=True, **D64),
    _case("published_256_64x16x16", H=16, W=16, inst=PHASE % "8,4", C=(256,), Cout=256, expect_split=True, **D64),
    _case("published_128_64x32x32", H=32, W=32, inst=PHASE % "8,4", C=(128,), Cout=128, **D64),
    _case("published_128_64x64x64", H=64, W=64, inst=PHASE % "8,4", C=(128,), Cout=128, **D64),
]
# shapes whose low-resolution grid does not tile like the output grid: the hinted call runs the 36-tap path
FALLBACK = [
    _case("fallback_w24", D=4, H=16, W=24, inst=PLAIN % "8,4"),
    _case("fallback_d1_8x8", D=1, H=8, W=8, inst=PLAIN % "8,8", res_mode="up"),
]


def n_acc(c):
    """m of the phase form: 2 x 2 taps per input channel and accumulator"""
    cinpad = -(-sum(c.C) // 16) * 16
    return 3 * 4 * cinpad + max(c.split, 1) + 8 + (16 if c.expect_split else 0)


def elem_bound(c, em):
    e_acc = 8.0 * U * torch.sqrt(n_acc(c) * em["sqterms"] / 3.0) + 2 * U * (em["trabs"] + em["out"].abs())
    return e_acc + em["silu"]


@functools.lru_cache(maxsize=2)
def _inputs(name):
    return G.inputs(next(c for c in CASES + FALLBACK if c.name == name))


def emulate_phase(c, t, pmut=None, **mut):
    return UE.conv32_up(t["srcs"], t["w"], t["b"], aff=t["aff"], act=c.act, bound=t["bound"], res=t["res"],
                        res_mode=c.res_mode, mut=E.Mut(**mut), pmut=pmut)


@pytest.fixture(scope="module")
def hc():
    import hipcall
    return hipcall


def run_gpu(hc, c, t, phase=True):
    """G.run_gpu with the phase image and DDPM3D_HINT_UP_PHASE; also checks the statistics rows and the workspace
    against the shape-only queries (hipcall.conv3d skips that for hinted calls)"""
    import guided_diffusion._hip as H
    lib = H.load()

    def pack_phase(w, precision=0):
        assert precision == 3
        co, ci = w.shape[0], w.shape[1]
        out = torch.empty(lib.ddpm3d_packed_up_phase_bytes(co, ci), dtype=torch.uint8, device=w.device)
        wc = w.contiguous()
        H.check(lib.ddpm3d_pack_up_phase_weight(H.ptr(wc), co, ci, H.ptr(out), H.stream()))
        torch.cuda.synchronize()
        return out

    kw = dict(in_mode=G.IN["up"], act=int(c.act), precision=3, bound=t["bound"].cuda(), want_stats=c.stats,
              hint=(c.split << H.HINT_SPLITK_SHIFT) | (H.HINT_UP_PHASE if phase else 0))
    if t["aff"] is not None:
        kw["aff"] = (t["aff"][0].cuda(), t["aff"][1].cuda())
    if t["res"] is not None:
        kw.update(res=hc.to_ndhwc(t["res"]).cuda(), res_mode=G.RES[c.res_mode])
    keep = hc.pack
    if phase:
        hc.pack = pack_phase
    try:
        out, stats, rows = hc.conv3d([hc.to_ndhwc(s).cuda() for s in t["srcs"]], t["w"].cuda(), t["b"].cuda(),
                                     (c.D, c.H, c.W), **kw)
    finally:
        hc.pack = keep
    plan = dict(hc.LAST_PLAN)
    if not c.split:
        cin = sum(c.C)
        assert rows == lib.ddpm3d_conv_stats_rows(c.N, c.D, c.H, c.W, cin, c.Cout, 3, 3)
        need = lib.ddpm3d_conv_workspace_bytes(c.N, c.D, c.H, c.W, cin, c.Cout, 3, 3)
        assert need == (plan["split"] * c.N * c.D * c.H * c.W * c.Cout * 4 if plan["split"] > 1 else 0)
    return out.cpu(), hc.to_ncdhw(out.cpu()).double(), (stats.cpu() if stats is not None else None), plan


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_up_phase_kernel_vs_emulation(hc, c):
    t = _inputs(c.name)
    out, got, stats, plan = run_gpu(hc, c, t)
    assert plan["family"] == c.family, (plan["family"], c.family)
    assert plan["instance"] == c.inst, (plan["instance"], c.inst)
    assert (plan["split"] > 1) == c.expect_split, plan
    if c.split:
        assert plan["split"] == c.split
    out2, _, stats2, _ = run_gpu(hc, c, t)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(stats.view(torch.int64), stats2.view(torch.int64))
    # the phase form ran: the unhinted call on the same inputs rounds its weights differently
    out36, got36, _, plan36 = run_gpu(hc, c, t, phase=False)
    assert plan36["split"] == plan["split"] and plan36["rows"] == plan["rows"]
    assert plan36["instance"] == G.G16.claimed_instance(c), (plan36["instance"], c.wz)
    assert not torch.equal(out.view(torch.int32), out36.view(torch.int32))
    assert torch.isfinite(got).all()
    # ---- against the emulation of the phase arithmetic
    em = emulate_phase(c, t)
    B = elem_bound(c, em)
    slack = U * em["out"].abs()
    err = (got - em["out"]).abs()
    print("%s: max |got - phase emulation| / bound %.3g" % (c.name, float((err / (B + slack)).max())))
    bad = err > B + slack
    assert not bad.any(), G.G16._where(bad, got=got, emul=em["out"], bound=B, silu=em["silu"])
    # GroupNorm partial sums of the fp32 result, fp64
    s = stats.double().sum(dim=2)
    y = em["out"]
    tol1 = B.sum(dim=(2, 3, 4)) + 1e-300
    tol2 = (2 * y.abs() * B + B * B).sum(dim=(2, 3, 4)) + 1e-300
    assert ((s[..., 0] - y.sum(dim=(2, 3, 4))).abs() <= tol1 * 1.0001 + 1e-12 * y.abs().sum(dim=(2, 3, 4))).all()
    assert ((s[..., 1] - (y * y).sum(dim=(2, 3, 4))).abs()
            <= tol2 * 1.0001 + 1e-12 * (y * y).sum(dim=(2, 3, 4))).all()
    del em, B, err
    # ---- results stay what they were: within the 36-tap kernel's own bar around the 36-tap form's emulation
    em36 = G.emulate(c, t)
    B36 = G.elem_bound(c, em36)
    err36 = (got - em36["out"]).abs()
    print("%s: max |got - 36-tap emulation| / its bound %.3g; 36-tap kernel %.3g" % (
        c.name, float((err36 / (B36 + U * em36["out"].abs())).max()),
        float(((got36 - em36["out"]).abs() / (B36 + U * em36["out"].abs())).max())))
    bad = err36 > B36 + U * em36["out"].abs()
    assert not bad.any(), G.G16._where(bad, got=got, emul=em36["out"], bound=B36, silu=em36["silu"])


@pytest.mark.parametrize("c", FALLBACK, ids=[c.name for c in FALLBACK])
def test_up_phase_fallback_is_the_shipped_path(hc, c):
    """the hint on a shape the phase form does not tile: the 36-tap path on the image's front part, bit for bit"""
    t = _inputs(c.name)
    out, _, stats, plan = run_gpu(hc, c, t)
    out36, _, stats36, plan36 = run_gpu(hc, c, t, phase=False)
    assert plan == plan36 and plan["instance"] == c.inst, (plan, plan36, c.inst)
    assert torch.equal(out.view(torch.int32), out36.view(torch.int32))
    assert torch.equal(stats.view(torch.int64), stats36.view(torch.int64))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_up_phase_error_against_fp64_within_twice_f32(hc, c):
    """test_gpu_conv32.test_f16x3_error_against_fp64_within_twice_f32's formula on the phase form"""
    t = _inputs(c.name)
    _, got, _, _ = run_gpu(hc, c, t)
    _, got0, _, _ = G.run_gpu(hc, dataclasses.replace(c, prec=0), t)
    ref = emulate_phase(c, t, exact=True)["out"]
    e_x3 = (got - ref).abs().amax(dim=(2, 3, 4))
    e_32 = (got0 - ref).abs().amax(dim=(2, 3, 4))
    top = ref.abs().amax(dim=(2, 3, 4))
    ratio = e_x3 / (e_32 + 1e-300)
    print("%s: phase f16x3 / f32 error per (sample, cout): median %.3g, max %.3g; worst err / max|ref| %.3g" % (
        c.name, float(ratio.median()), float(ratio.max()), float((e_x3 / top.clamp_min(1e-300)).max())))
    bad = e_x3 > 2 * e_32 + 4 * U * top
    assert not bad.any(), [(tuple(i), float(e_x3[tuple(i)]), float(e_32[tuple(i)]), float(top[tuple(i)]))
                           for i in bad.nonzero()[:6].tolist()]
