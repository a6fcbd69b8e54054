"""
p_mean_variance and DDIM inversion on the GPU (gaussian_diffusion.py:232-326, :587-623, and the package's
ddim_reverse_sample_loop) against the reference's own outputs (tests/golden/ddim_reverse.npz,
make_golden_ddim_reverse.py), an fp64 restatement written here, and itself (repeatability, the step graph, the
direct per-step call).

Kernel-level bars (one fixed model output, N = 3 volumes of 4x16x16 at t = [0, 125, 249] of "250"): every output
within 1e-5 of the reference (max |a - b| / max |b| per tensor); variance may differ by an ulp of expf from the
reference host's libm.  Measured on an MI355X: see the docstrings of the tests.
End to end: every step of the inversion loop within 1e-3 (the sampler loops' bar).
"""

import numpy as np
import pytest
import torch

from conftest import rel_err
from guided_diffusion import _hip as H
from guided_diffusion import script_util as su
from guided_diffusion import synth

pytestmark = pytest.mark.gpu

PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True,
                 use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)
SEEDS = dict(x=22, model_output=23, x_start=21, low_res=1234)          # make_golden_ddim_reverse.SEEDS
K_SHAPE = (3, 1, 4, 16, 16)
K_VARIANTS = {"learned_range": dict(learn_sigma=True), "fixed_large": dict(learn_sigma=False),
              "fixed_small": dict(learn_sigma=False, sigma_small=True),
              "xstart": dict(learn_sigma=True, predict_xstart=True)}
E_CASES = {"tiny": (TINY, (2, 1, 4, 16, 16), {}),
           "tiny_noclip": (TINY, (1, 1, 4, 16, 16), dict(clip_denoised=False)),
           "tiny_nosigma": (dict(TINY, learn_sigma=False), (1, 1, 4, 16, 16), {}),
           "tiny_xstart": (dict(TINY, predict_xstart=True), (1, 1, 4, 16, 16), {}),
           "published": (PUBLISHED, (1, 1, 8, 32, 32), {})}


def build(over, resp, precision=None):
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(over)
    fl["timestep_respacing"] = resp
    model, diff = su.sr_create_model_and_diffusion(**fl)
    if precision is not None:
        model.conv_precision = precision
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape))) for k, v in sd.items()})
    model.to("cuda").eval()
    return model, diff


def np_(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("variant", sorted(K_VARIANTS))
def test_kernels_vs_reference(golden, variant, clip):
    """p_mean_variance's four outputs and ddim_reverse_sample's two against the reference's.  Measured on an
    MI355X, all eight cases: mean, pred_xstart, sample and log_variance bitwise (0.0); the fixed variances bitwise;
    the learned variance 4.8e-8 (expf within an ulp of the reference host's exp)."""
    g = golden("ddim_reverse.npz")
    key = "k/%s/%s" % (variant, "clip" if clip else "noclip")
    over = K_VARIANTS[variant]
    d = su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", **over)
    x = torch.from_numpy(synth.synth_noise(K_SHAPE, 1, seed=SEEDS["x"])[0]).cuda()
    mo = torch.from_numpy(synth.synth_model_output(K_SHAPE, over["learn_sigma"], SEEDS["model_output"])).cuda()
    t = torch.from_numpy(g["k/t"])
    calls = []

    def model(xx, tt, **kw):
        calls.append(tt)
        return mo

    pmv = d.p_mean_variance(model, x, t, clip_denoised=clip)
    rev = d.ddim_reverse_sample(model, x, t, clip_denoised=clip)
    assert len(calls) == 2
    for k in ("mean", "variance", "log_variance", "pred_xstart"):
        assert pmv[k].is_cuda and pmv[k].dtype == torch.float32 and pmv[k].shape == x.shape, k
    assert torch.equal(rev["pred_xstart"], pmv["pred_xstart"])
    errs = {k: rel_err(np_(pmv[k]), g[key + "/" + k]) for k in ("mean", "pred_xstart")}
    errs["sample"] = rel_err(np_(rev["sample"]), g[key + "/sample"])
    if over["learn_sigma"]:
        for k in ("variance", "log_variance"):
            errs[k] = rel_err(np_(pmv[k]), g[key + "/" + k])
        # expf against the reference's fp32 exp: an ulp at most, voxel by voxel
        ulp = np.spacing(np.abs(g[key + "/variance"]))
        assert (np.abs(np_(pmv["variance"]) - g[key + "/variance"]) <= ulp).all()
    else:
        for k in ("variance", "log_variance"):
            v = np_(pmv[k]).reshape(K_SHAPE[0], -1)
            assert (v == v[:, :1]).all(), k                         # one value per sample, expanded
            assert np.array_equal(v[:, 0], g[key + "/" + k]), k      # the fp64 table at t, rounded once
            errs[k] = 0.0
    print(key, " ".join("%s %.2e" % kv for kv in sorted(errs.items())))
    assert max(errs.values()) < 1e-5, errs


def restate(diff, mo, x, t, clip=True, dtype=torch.float64):
    """The reverse step and p_mean_variance in torch on the GPU (fp64 by default) from the fp32 table the library
    reads.  x: (N, C, ...), mo: (N, 2C or C, ...), split along channels as the reference does (:264)."""
    coef = torch.from_numpy(diff.coef_table()).cuda().to(dtype)
    T = diff.num_timesteps
    tc = t.cuda().long()
    row = coef[tc]
    nxt = torch.where(tc + 1 < T, coef[(tc + 1).clamp(max=T - 1), 6], torch.zeros((), dtype=dtype, device="cuda"))
    b = (-1,) + (1,) * (x.dim() - 1)
    c_recip, c_recipm1, c1, c2, min_log, max_log = (row[:, j].reshape(b) for j in range(6))
    ab_next = nxt.reshape(b)
    C = x.shape[1]
    x = x.to(dtype)
    eps_in = mo[:, :C].to(dtype)
    x0 = eps_in if diff.model_mean_type.name == "START_X" else c_recip * x - c_recipm1 * eps_in
    if clip:
        x0 = x0.clamp(-1, 1)
    eps = (c_recip * x - x0) / c_recipm1
    sample = x0 * torch.sqrt(ab_next) + torch.sqrt(1 - ab_next) * eps
    out = {"sample": sample, "pred_xstart": x0, "mean": c1 * x0 + c2 * x, "eps": eps}
    if mo.shape[1] == 2 * C:
        frac = (mo[:, C:].to(dtype) + 1) / 2
        out["log_variance"] = frac * max_log + (1 - frac) * min_log
        out["variance"] = torch.exp(out["log_variance"])
    return out


@pytest.mark.parametrize("clip", [True, False])
def test_reverse_step_vs_restatement(clip):
    """The "ddim50" schedule at t = [0, 1, 24, 48, 49], N = 5 volumes of 8x16x16.  Measured on an MI355X: vs the
    same expressions in fp32 torch, bitwise (0.0); vs fp64 every output <= 2.4e-7 (max-norm relative) except the
    clipped pred_xstart, 1.04e-5.  That one is the reference's fp32 expression itself: at t = 49,
    sqrt_recip_acp * x - sqrt_recipm1_acp * eps subtracts two products of ~130 |x| and keeps a result clipped to
    [-1, 1], so fp32 rounding of the products (~1e-5 absolute) is all that is left; the fp32 torch restatement sits
    at the same distance from fp64.  The fp64 bar is therefore 1e-5 or the fp32 expression's own distance plus
    1e-6, whichever is larger.  At t = T - 1, ab_next = 0 and the sample is the recomputed eps itself, bitwise."""
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="ddim50")
    T = d.num_timesteps
    shape = (5, 1, 8, 16, 16)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=41)[0]).cuda()
    mo = torch.from_numpy(synth.synth_model_output(shape, True, 42)).cuda()
    t = torch.tensor([0, 1, T // 2 - 1, T - 2, T - 1])
    rev = d.ddim_reverse_sample(lambda *a, **k: mo, x, t, clip_denoised=clip)
    pmv = d.p_mean_variance(lambda *a, **k: mo, x, t, clip_denoised=clip)
    r64 = restate(d, mo, x, t, clip)
    r32 = restate(d, mo, x, t, clip, dtype=torch.float32)
    got = {"sample": rev["sample"], "pred_xstart": rev["pred_xstart"], "mean": pmv["mean"],
           "log_variance": pmv["log_variance"], "variance": pmv["variance"]}
    e64 = {k: rel_err(np_(v), np_(r64[k])) for k, v in got.items()}
    e32 = {k: rel_err(np_(v), np_(r32[k])) for k, v in got.items()}
    print("clip=%s vs fp64: %s; vs fp32 torch: %s" % (clip, e64, e32))
    assert max(e32[k] for k in ("sample", "pred_xstart", "mean", "log_variance")) < 1e-6, e32
    for k in got:
        own = rel_err(np_(r32[k]), np_(r64[k]))           # the fp32 expression's own distance from fp64
        assert e64[k] < max(1e-5, own + 1e-6), (k, e64[k], own)
    # t = T - 1: sample == eps recomputed from pred_xstart in fp32, bit for bit
    coef = torch.from_numpy(d.coef_table()).cuda()[T - 1]
    eps = (coef[0] * x[4] - rev["pred_xstart"][4]) / coef[1]
    assert torch.equal(rev["sample"][4], eps)


def test_two_dimensional_three_channel_step():
    """A 2-D (N, 3, H, W) input: voxels spans the channels, as for the samplers; mo's first three channels are
    eps and the next three the variance fractions."""
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="250")
    shape = (2, 3, 16, 16)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=51)[0]).cuda()
    mo = torch.from_numpy(synth.synth_model_output(shape, True, 52)).cuda()
    assert mo.shape == (2, 6, 16, 16)
    t = torch.tensor([7, 200])
    rev = d.ddim_reverse_sample(lambda *a, **k: mo, x, t)
    pmv = d.p_mean_variance(lambda *a, **k: mo, x, t)
    r = restate(d, mo, x, t)
    for k, v in (("sample", rev["sample"]), ("pred_xstart", rev["pred_xstart"]), ("mean", pmv["mean"]),
                 ("log_variance", pmv["log_variance"]), ("variance", pmv["variance"])):
        assert v.shape == x.shape, k
        err = rel_err(np_(v), np_(r[k]))
        assert err < 1e-5, (k, err)


def test_out_of_range_t():
    """The Python layer raises ValueError before the model runs; the kernels themselves answer NaN for that sample
    only, without reading a table row."""
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="10")
    x = torch.from_numpy(synth.synth_noise((2, 1, 4, 8, 8), 1, seed=5)[0]).cuda()
    mo = torch.from_numpy(synth.synth_model_output((2, 1, 4, 8, 8), True, 6)).cuda()
    calls = []

    def model(xx, tt, **kw):
        calls.append(1)
        return mo[:xx.shape[0]]

    for bad in ([0, 10], [-1, 3], [0]):
        with pytest.raises(ValueError):
            d.p_mean_variance(model, x, torch.tensor(bad))
        with pytest.raises(ValueError):
            d.ddim_reverse_sample(model, x, torch.tensor(bad))
    assert not calls
    lib = H.load()
    st = d._device_state(x.device)
    t = torch.tensor([3, 10], device="cuda")
    vox = x[0].numel()
    good = d.ddim_reverse_sample(model, x[:1], torch.tensor([3]))
    sample, x0 = torch.zeros_like(x), torch.zeros_like(x)
    H.check(lib.ddpm3d_ddim_reverse_step(H.ptr(mo), H.ptr(x), H.ptr(st["coef"]), H.ptr(t), 2, vox, 10,
                                         H.F_LEARN_SIGMA | H.F_CLIP, H.ptr(sample), H.ptr(x0), H.stream()))
    assert torch.equal(sample[:1], good["sample"]) and torch.equal(x0[:1], good["pred_xstart"])
    assert torch.isnan(sample[1]).all() and torch.isnan(x0[1]).all()
    pm = d.p_mean_variance(model, x[:1], torch.tensor([3]))
    outs = [torch.zeros_like(x) for _ in range(4)]
    H.check(lib.ddpm3d_p_mean_variance(H.ptr(mo), H.ptr(x), H.ptr(st["coef"]), H.ptr(t), 2, vox, 10,
                                       H.F_LEARN_SIGMA | H.F_CLIP, *(H.ptr(o) for o in outs), H.stream()))
    for o, k in zip(outs, ("mean", "variance", "log_variance", "pred_xstart")):
        assert torch.equal(o[:1], pm[k]) and torch.isnan(o[1]).all(), k


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("tag", sorted(E_CASES))
def test_inversion_loop_vs_reference(golden, tag, precision):
    """ddim_reverse_sample_loop on "ddim10" against the reference's ddim_reverse_sample written out as a loop,
    every stored sample within 1e-3 (max-norm relative).  Measured on an MI355X, worst step of the ten: tiny
    1.0e-5 (f32) / 7.3e-6 (f16x3), tiny_noclip 2.8e-5 / 1.3e-5, tiny_nosigma 1.0e-5 / 6.3e-6, tiny_xstart
    3.7e-6 / 2.1e-6; published x_T 7.7e-6 / 7.2e-6.

    The published case's last pred_xstart is held to the bar relative to the largest term it is formed from,
    sqrt_recip_acp[T-1] * max |x_{T-1}|, not to its own maximum.  At t = T - 1, pred_xstart = 60.8 x - 60.8 eps
    (sqrt_recip_acp of "ddim10"), clipped to [-1, 1]: the step's input, which after nine forwards already differs
    from the reference's by ~7e-6 (CPU against GPU summation order), and the network's eps reach pred_xstart
    multiplied by 60.8, while its maximum is the clip bound.  Measured on an MI355X, relative to its own maximum it
    is 1.1e-3 (f32) / 1.2e-3 (f16x3) from the reference -- the same in both modes, so not the mode's rounding; the
    kernel's own arithmetic is bitwise the reference's (test_kernels_vs_reference).  Relative to the term it is
    formed from: 6.7e-6 (f32) / 7.2e-6 (f16x3)."""
    over, shape, kw = E_CASES[tag]
    model, diff = build(over, "ddim10", precision)
    xs = torch.from_numpy(synth.synth_x_start(shape, SEEDS["x_start"])).cuda()
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=SEEDS["low_res"])).cuda()
    g = golden("ddim_reverse.npz")
    steps = list(diff.ddim_reverse_sample_loop_progressive(model, xs, model_kwargs={"low_res": lr}, **kw))
    assert len(steps) == diff.num_timesteps == 10
    if tag == "published":
        # pred_xstart against the largest term it is formed from, sqrt_recip_acp[T-1] * max |x_{T-1}|
        px = np_(steps[-1]["pred_xstart"]).astype(np.float64)
        scale = diff.sqrt_recip_alphas_cumprod[-1] * float(steps[-2]["sample"].abs().max())
        errs = [rel_err(np_(steps[-1]["sample"]), g["e/published/sample"]),
                float(np.abs(px - g["e/published/pred_xstart"]).max() / scale)]
        print("published %s: pred_xstart max rel err %.2e to its own maximum"
              % (precision, rel_err(px, g["e/published/pred_xstart"])))
    else:
        ref = g["e/%s/samples" % tag]
        errs = [rel_err(np_(s["sample"]), ref[k]) for k, s in enumerate(steps)]
    final = diff.ddim_reverse_sample_loop(model, xs, model_kwargs={"low_res": lr}, **kw)
    assert torch.equal(final, steps[-1]["sample"])
    print("%s %s: max rel err per step %s" % (tag, precision, " ".join("%.1e" % e for e in errs)))
    assert max(errs) < 1e-3, (tag, precision, errs)


def test_published_64_inversion_properties():
    """The published network at 1 x 64^3, "ddim50": two runs bitwise equal; the progressive form's step k is
    exactly one ddim_reverse_sample(model, ...) call on step k - 1's sample (k = 0, 25, 49); the step graph gives
    the eager bits, and a graph really ran."""
    model, diff = build(PUBLISHED, "ddim50")
    T = diff.num_timesteps
    shape = (1, 1, 64, 64, 64)
    xs = torch.from_numpy(synth.synth_x_start(shape, SEEDS["x_start"])).cuda()
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=SEEDS["low_res"])).cuda()
    kw = {"low_res": lr}
    keep = {-1: xs}
    for k, r in enumerate(diff.ddim_reverse_sample_loop_progressive(model, xs, model_kwargs=kw)):
        if k in (0, 24, 25, 48, 49):
            keep[k] = r["sample"]
    a = keep[T - 1]
    assert torch.isfinite(a).all()
    b = diff.ddim_reverse_sample_loop(model, xs, model_kwargs=kw)
    assert torch.equal(a, b)
    for k in (0, 25, 49):
        one = diff.ddim_reverse_sample(model, keep[k - 1], torch.tensor([k]), model_kwargs=kw)
        assert torch.equal(one["sample"], keep[k]), k
    del keep, b
    model.step_graph = True
    try:
        c = diff.ddim_reverse_sample_loop(model, xs, model_kwargs=kw)
        eng = model.engine()
        assert eng.step_graph and any(pl.graphs for pl in eng.plans.values())      # the graph path really ran
    finally:
        model.step_graph = False
    assert torch.equal(a, c)
