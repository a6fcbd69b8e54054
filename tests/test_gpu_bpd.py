"""
The variational bound on the GPU (q_sample, _vb_terms_bpd, _prior_bpd, calc_bpd_loop; gaussian_diffusion.py:171-230,
:709-742, :821-894) against the reference's own outputs (tests/golden/bpd.npz, make_golden_bpd.py), an fp64
restatement written here, and itself (repeatability, step graph, the direct per-step call).

Kernel-level bars (one fixed model output, N = 3 volumes of 16x32x32 at t = [0, 125, 249] of "250"):
  q_sample      bitwise: the same two fp32 products and one sum as the reference, no contraction;
  KL, MSEs, prior 1e-5 relative per sample; decoder NLL (t = 0) 1e-4 relative.
The kernel evaluates exp / log / tanh in fp64 and rounds once (the correctly rounded fp32 value); the reference's
fp32 libm is within 1 ulp of it, and the remaining differences are those ulps and the fp64-vs-fp32 order of the
per-sample mean.  Measured on an MI355X, max over the six variants: NLL 2.0e-7, KL 2.4e-7, xstart_mse 1.8e-7,
mse 1.2e-7, prior 9.0e-8 -- the bars leave room for another host's libm.
End to end: every entry of all five calc_bpd_loop outputs within 1e-3 relative (the sampler loops' bar); measured
<= 2.1e-5 (vb of the predict_xstart network), <= 1e-6 for the other outputs, in f16x3 and f32 alike.
"""

import numpy as np
import pytest
import torch

from guided_diffusion import _hip as H
from guided_diffusion import script_util as su
from guided_diffusion import synth

pytestmark = pytest.mark.gpu

PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True,
                 use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)
SEEDS = dict(x_start=21, noise=22, model_output=23, low_res=1234, steps=10)      # make_golden_bpd.SEEDS
K_SHAPE = (3, 1, 16, 32, 32)
K_VARIANTS = {"learned_range": dict(learn_sigma=True), "fixed_large": dict(learn_sigma=False),
              "xstart": dict(learn_sigma=True, predict_xstart=True)}
E_CASES = {"tiny10": (TINY, (2, 1, 8, 16, 16), {}),
           "tiny10_nosigma": (dict(TINY, learn_sigma=False), (1, 1, 4, 16, 16), {}),
           "tiny10_noclip": (TINY, (1, 1, 4, 16, 16), dict(clip_denoised=False)),
           "tiny10_xstart": (dict(TINY, predict_xstart=True), (1, 1, 4, 16, 16), {}),
           "published10": (PUBLISHED, (1, 1, 8, 32, 32), {})}
OUTPUTS = ["total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"]


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


def rel(a, b):
    """per-entry |a - b| / |b|"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def kernel_inputs():
    xs = torch.from_numpy(synth.synth_x_start(K_SHAPE, SEEDS["x_start"])).cuda()
    noise = torch.from_numpy(synth.synth_noise(K_SHAPE, 1, seed=SEEDS["noise"])[0]).cuda()
    return xs, noise


def all_terms(diff, mo, xs, xt, t, noise, clip):
    """vb, xstart_mse, mse [N] and pred_xstart of one ddpm3d_vb_terms launch."""
    N = xs.shape[0]
    vb, xm, mse = (torch.full((N,), float("nan"), device="cuda") for _ in range(3))
    x0 = torch.empty_like(xs)
    t = t.cuda().long().contiguous()
    diff._vb_terms(mo, xs, xt, t, noise, diff._flags(clip), diff._workspace(xs), vb, xm, mse, 1, x0)
    return vb, xm, mse, x0


def test_q_sample_and_prior_vs_reference(golden):
    g = golden("bpd.npz")
    xs, noise = kernel_inputs()
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="250")
    t = torch.from_numpy(g["k/t"])
    xt = d.q_sample(xs, t, noise=noise)
    assert xt.shape == xs.shape and xt.dtype == torch.float32 and xt.is_cuda
    assert np.array_equal(xt.cpu().numpy(), g["k/q_sample"])
    prior = d._prior_bpd(xs)
    err = rel(prior.cpu().numpy(), g["k/prior_bpd"]).max()
    print("prior_bpd max rel err %.2e" % err)
    assert err < 1e-5


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("variant", sorted(K_VARIANTS))
def test_vb_terms_vs_reference(golden, variant, clip):
    g = golden("bpd.npz")
    key = "k/%s/%s" % (variant, "clip" if clip else "noclip")
    over = K_VARIANTS[variant]
    d = su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", **over)
    xs, noise = kernel_inputs()
    xt = torch.from_numpy(g["k/q_sample"]).cuda()
    t = torch.from_numpy(g["k/t"])
    mo = torch.from_numpy(synth.synth_model_output(K_SHAPE, over["learn_sigma"], SEEDS["model_output"])).cuda()
    vb, xm, mse, x0 = all_terms(d, mo, xs, xt, t, noise, clip)
    e_nll = rel(vb[0].item(), g[key + "/vb"][0])
    e_kl = rel(vb[1:].cpu().numpy(), g[key + "/vb"][1:]).max()
    e_xm = rel(xm.cpu().numpy(), g[key + "/xstart_mse"]).max()
    e_mse = rel(mse.cpu().numpy(), g[key + "/mse"]).max()
    print("%s: nll %.2e kl %.2e xstart_mse %.2e mse %.2e" % (key, e_nll, e_kl, e_xm, e_mse))
    assert e_nll < 1e-4 and e_kl < 1e-5 and e_xm < 1e-5 and e_mse < 1e-5
    # the public call: same kernel, same bits, pred_xstart included
    r = d._vb_terms_bpd(lambda *a, **k: mo, xs, xt, t, clip_denoised=clip)
    assert torch.equal(r["output"], vb) and torch.equal(r["pred_xstart"], x0)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("tag", sorted(E_CASES))
def test_calc_bpd_loop_vs_reference(golden, tag, precision):
    over, shape, kw = E_CASES[tag]
    model, diff = build(over, "10", precision)
    T = diff.num_timesteps
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, T, seed=SEEDS["steps"])]
    xs = torch.from_numpy(synth.synth_x_start(shape, SEEDS["x_start"])).cuda()
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=SEEDS["low_res"])).cuda()
    r = diff.calc_bpd_loop(model, xs, model_kwargs={"low_res": lr}, step_noise=draws, **kw)
    g = golden("bpd.npz")
    for k in OUTPUTS:
        ref = g["e/%s/%s" % (tag, k)]
        got = r[k]
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape, k
        err = rel(got.cpu().numpy(), ref).max()
        print("%s %s %s: max rel err %.2e" % (tag, precision, k, err))
        assert err < 1e-3, (tag, precision, k, err)


def restate(diff, mo, xs, xt, noise, t, clip=True, dtype=torch.float64):
    """The bound's terms in torch on the GPU (fp64 by default), from the fp32 tables the library reads."""
    coef = torch.from_numpy(diff.coef_table()).cuda().to(dtype)[t]
    q = torch.from_numpy(diff.qcoef_table()).cuda().to(dtype)[t]
    b = (-1, 1, 1, 1, 1)
    c_recip, c_recipm1, c1, c2, min_log, max_log = (coef[:, j].reshape(b) for j in range(6))
    true_log = q[:, 3].reshape(b)
    mo, xs, xt, noise = mo.to(dtype), xs.to(dtype), xt.to(dtype), noise.to(dtype)
    eps = mo[:, :1]
    x0 = c_recip * xt - c_recipm1 * eps
    if clip:
        x0 = x0.clamp(-1, 1)
    frac = (mo[:, 1:] + 1) / 2
    logvar = frac * max_log + (1 - frac) * min_log
    mean = c1 * x0 + c2 * xt
    tmean = c1 * xs + c2 * xt
    kl = 0.5 * (-1.0 + logvar - true_log + torch.exp(true_log - logvar) + (tmean - mean) ** 2 * torch.exp(-logvar))

    def cdf(x):
        return 0.5 * (1.0 + torch.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))

    inv_stdv = torch.exp(-0.5 * logvar)
    cdf_plus = cdf(inv_stdv * (xs - mean + 1.0 / 255.0))
    cdf_min = cdf(inv_stdv * (xs - mean - 1.0 / 255.0))
    lp = torch.where(xs < -0.999, torch.log(cdf_plus.clamp(min=1e-12)),
                     torch.where(xs > 0.999, torch.log((1.0 - cdf_min).clamp(min=1e-12)),
                                 torch.log((cdf_plus - cdf_min).clamp(min=1e-12))))
    dims = (1, 2, 3, 4)
    vb = torch.where(t.cuda() == 0, (-lp).double().mean(dims), kl.double().mean(dims)) / np.log(2.0)
    eps_x0 = (c_recip * xt - x0) / c_recipm1
    return vb, ((x0 - xs) ** 2).double().mean(dims), ((eps_x0 - noise) ** 2).double().mean(dims)


def test_published_64_bound_properties():
    """The published network at 1 x 64^3, "50": repeatability, the sum, the per-step identity with _vb_terms_bpd,
    and, at N = 2 with t = [0, 20], the terms against the restatement above from the same model output.
    Measured on an MI355X: vs fp64 the t = 0 NLL 1.53e-5 (the fp32 torch restatement: 1.53e-5 as well), the
    t = 20 KL 1.1e-7, the MSEs <= 2.0e-8; vs the fp32 torch restatement every term <= 6.8e-8."""
    model, diff = build(PUBLISHED, "50")
    T = diff.num_timesteps
    shape = (1, 1, 64, 64, 64)
    xs = torch.from_numpy(synth.synth_x_start(shape, SEEDS["x_start"])).cuda()
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=SEEDS["low_res"])).cuda()
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, T, seed=SEEDS["steps"])]
    kw = {"low_res": lr}
    a = diff.calc_bpd_loop(model, xs, model_kwargs=kw, step_noise=draws)
    b = diff.calc_bpd_loop(model, xs, model_kwargs=kw, step_noise=lambda k, x: draws[k])
    for k in OUTPUTS:
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k
    assert tuple(a["vb"].shape) == (1, T) and tuple(a["total_bpd"].shape) == (1,)
    assert torch.equal(a["total_bpd"], a["vb"].sum(1) + a["prior_bpd"])
    assert torch.equal(a["prior_bpd"], diff._prior_bpd(xs))
    for k in (0, T // 2, T - 1):                     # column k is step t = T - 1 - k
        t = torch.full((1,), T - 1 - k, dtype=torch.long, device="cuda")
        xt = diff.q_sample(xs, t, noise=draws[k])
        r = diff._vb_terms_bpd(model, xs, xt, t, model_kwargs=kw)
        assert torch.equal(r["output"], a["vb"][:, k]), k
        _, xm, mse, _ = all_terms(diff, model(xt, diff._model_timesteps(t), **kw), xs, xt, t, draws[k], True)
        assert torch.equal(xm, a["xstart_mse"][:, k]) and torch.equal(mse, a["mse"][:, k]), k
    del a, b, draws
    # N = 2, mixed t including 0, against fp64
    shape2 = (2, 1, 64, 64, 64)
    xs2 = torch.from_numpy(synth.synth_x_start(shape2, 31)).cuda()
    lr2 = torch.from_numpy(synth.synth_low_res(shape2, seed=32)).cuda()
    noise2 = torch.from_numpy(synth.synth_noise(shape2, 1, seed=33)[0]).cuda()
    t2 = torch.tensor([0, 20], device="cuda")
    xt2 = diff.q_sample(xs2, t2, noise=noise2)
    mo = model(xt2, diff._model_timesteps(t2), low_res=lr2).clone()
    vb, xm, mse, _ = all_terms(diff, mo, xs2, xt2, t2, noise2, True)
    got = [x.cpu().numpy() for x in (vb, xm, mse)]
    r64 = [x.cpu().numpy() for x in restate(diff, mo, xs2, xt2, noise2, t2)]
    r32 = [x.cpu().numpy() for x in restate(diff, mo, xs2, xt2, noise2, t2, dtype=torch.float32)]
    e64 = [rel(a, b) for a, b in zip(got, r64)]
    e32 = [rel(a, b).max() for a, b in zip(got, r32)]
    print("published 64^3 vs fp64: nll %.2e kl %.2e xstart_mse %.2e mse %.2e; vs fp32 torch: %.2e %.2e %.2e"
          % (e64[0][0], e64[0][1], e64[1].max(), e64[2].max(), *e32))
    # fp64: the KL and the MSEs 1e-5; the t = 0 NLL 1e-4, because the reference's fp32 expression itself sits
    # 1.5e-5 from fp64 there (cdf_plus - cdf_min cancels) -- measured, as is the kernel's 6.7e-8 from that fp32
    # expression evaluated by torch on the same data, which is what the second bar holds it to
    assert e64[0][0] < 1e-4 and e64[0][1] < 1e-5 and e64[1].max() < 1e-5 and e64[2].max() < 1e-5, e64
    assert max(e32) < 1e-6, e32


def test_calc_bpd_loop_step_graph_equals_eager():
    model, diff = build(TINY, "10")
    shape = (2, 1, 8, 16, 16)
    xs = torch.from_numpy(synth.synth_x_start(shape, SEEDS["x_start"])).cuda()
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=SEEDS["low_res"])).cuda()
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 10, seed=SEEDS["steps"])]
    res = {}
    for graph in (False, True):
        model.step_graph = graph
        res[graph] = diff.calc_bpd_loop(model, xs, model_kwargs={"low_res": lr}, step_noise=draws)
    eng = model.engine()
    assert eng.step_graph and any(pl.graphs for pl in eng.plans.values())      # the graph path really ran
    for k in OUTPUTS:
        assert torch.isfinite(res[False][k]).all() and torch.equal(res[False][k], res[True][k]), k


def test_out_of_range_t():
    """The Python layer raises before anything runs; the kernels themselves answer NaN without a table read."""
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="10")
    xs, noise = (torch.from_numpy(a).cuda() for a in synth.synth_noise((2, 1, 4, 8, 8), 2, seed=5))
    calls = []

    def model(x, t, **kw):
        calls.append(1)
        return torch.zeros((2, 2, 4, 8, 8), device="cuda")

    for bad in ([0, 10], [-1, 3], [0]):
        with pytest.raises(ValueError):
            d.q_sample(xs, torch.tensor(bad), noise=noise)
        with pytest.raises(ValueError):
            d._vb_terms_bpd(model, xs, xs, torch.tensor(bad))
        with pytest.raises(ValueError):
            d.q_mean_variance(xs, torch.tensor(bad))
    assert not calls
    # C ABI, device side: t = T reads no row (the tables have T rows) and yields NaN; the in-range sample is untouched
    lib = H.load()
    st = d._device_state(xs.device)
    t = torch.tensor([3, 10], device="cuda")
    xt = torch.zeros_like(xs)
    H.check(lib.ddpm3d_q_sample(H.ptr(xs), H.ptr(noise), H.ptr(st["qcoef"]), H.ptr(t), 2, xs[0].numel(), 10,
                                H.ptr(xt), H.stream()))
    good = d.q_sample(xs[:1], torch.tensor([3]), noise=noise[:1])
    assert torch.equal(xt[:1], good) and torch.isnan(xt[1]).all()
    mo = torch.zeros((2, 2, 4, 8, 8), device="cuda")
    vb, xm, mse, _ = all_terms(d, mo, xs, good.expand_as(xs).contiguous(), t, noise, True)
    assert torch.isfinite(vb[0]) and torch.isfinite(xm[0]) and torch.isfinite(mse[0])
    assert torch.isnan(vb[1]) and torch.isnan(xm[1]) and torch.isnan(mse[1])


def test_cpu_tensors_are_refused():
    model, diff = build(TINY, "10")
    xs = torch.from_numpy(synth.synth_x_start((1, 1, 4, 16, 16), SEEDS["x_start"]))
    lr = torch.from_numpy(synth.synth_low_res((1, 1, 4, 16, 16), seed=SEEDS["low_res"]))
    with pytest.raises(RuntimeError, match="GPU"):
        diff.calc_bpd_loop(model, xs, model_kwargs={"low_res": lr})
    with pytest.raises(RuntimeError, match="GPU"):
        diff.q_sample(xs, torch.tensor([1]))
    with pytest.raises(RuntimeError, match="GPU"):
        diff._prior_bpd(xs)
