"""
The DPM-Solver++ multistep sampler on the GPU (ddpm3d_dpm_solver_step, dpm_solver_sample_loop): the kernel against an
fp64 restatement of its weighted sum and, for pred_xstart, bitwise against the DDIM step; the loop at order 1 against
ddim_sample_loop (itself pinned to the reference's outputs), at orders 2 and 3 against the CPU oracle network plus an
fp64 solver, on an analytic Gaussian-data model against the exact ODE solution, and against itself across the
engine's launch paths.  Also the published network at 1 x 64^3 and the inference script.
"""

import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from conftest import PKG, rel_err
from guided_diffusion import _hip as H
from guided_diffusion import script_util as su
from guided_diffusion import synth
from test_dpm_solver_cpu import MU, SD, gaussian_exact, solve_gaussian

pytestmark = pytest.mark.gpu

PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True,
                 use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)
SOLVERS = [(1, False), (2, False), (3, False), (1, True), (2, True)]
VARIANTS = {"learned_range": dict(learn_sigma=True), "fixed": dict(learn_sigma=False),
            "xstart": dict(learn_sigma=True, predict_xstart=True)}


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def step(d, mo, x, m1, m2, z, t, flags, order, stochastic):
    """One ddpm3d_dpm_solver_step launch on the library's tables."""
    st = d._device_state(x.device)
    scoef = d._solver_state(x.device, order, stochastic)
    sample, x0 = torch.empty_like(x), torch.empty_like(x)
    t = torch.as_tensor(t, dtype=torch.int64).cuda()
    H.check(H.load().ddpm3d_dpm_solver_step(H.ptr(mo), H.ptr(x), H.ptr(m1), H.ptr(m2), H.ptr(z), H.ptr(st["coef"]),
                                            H.ptr(scoef), H.ptr(t), x.shape[0], x[0].numel(), d.num_timesteps, flags,
                                            order, H.ptr(sample),
                                            H.ptr(x0), H.stream()))
    return sample, x0


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("order,stochastic", SOLVERS)
def test_kernel_vs_fp64_restatement(order, stochastic, variant, clip):
    """N = 2 volumes at different t, among them the final row (t = 0).  sample against the fp32 table's weighted
    sum in fp64 of the kernel's own pred_xstart and inputs, per element within 6 fp32 ulps of
    |c_x x| + sum |w m| + |c_z z|; pred_xstart bitwise ddpm3d_ddim_step's; the final row returns pred_xstart
    exactly."""
    over = VARIANTS[variant]
    d = su.create_gaussian_diffusion(steps=1000, timestep_respacing="logsnr20", **over)
    flags = d._flags(clip)
    shape = (2, 1, 4, 16, 16)
    x, m1, m2, z = (dev(a) for a in synth.synth_noise(shape, 4, seed=61))
    mo = dev(synth.synth_model_output(shape, over["learn_sigma"], 62))
    m1, m2 = m1.clamp(-1, 1), m2.clamp(-1, 1)
    tab = d.dpm_solver_table(order, stochastic).astype(np.float64)
    for t in ([17, 4], [0, 9], [19, 0]):
        noise = z if stochastic else None
        sample, x0 = step(d, mo, x, m1, m2, noise, t, flags, order, stochastic)
        ddim = d._update("ddim", mo, x, torch.tensor(t), z, clip, 0.0)
        assert torch.equal(x0, ddim["pred_xstart"]), t
        terms = [np_(v).astype(np.float64) for v in (x, x0, m1, m2, z)]
        for n, ti in enumerate(t):
            w = tab[ti]
            used = [0, 1] + ([2] if order >= 2 else []) + ([3] if order == 3 else []) + ([4] if stochastic else [])
            parts = [w[j] * terms[j][n] for j in used]
            ref = sum(parts)
            bound = 6 * 2.0 ** -23 * sum(np.abs(p) for p in parts)
            assert (np.abs(np_(sample[n]) - ref) <= bound).all(), (t, n)
            if ti == 0:
                assert torch.equal(sample[n], x0[n])


def test_kernel_reads_history_and_noise_by_order():
    """At order 1 the kernel reads neither x0_prev1 nor x0_prev2: NaN-filled ones give the bits of NULL pointers;
    at order 2 a NaN-filled x0_prev2 is never read."""
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="logsnr10")
    shape = (1, 1, 4, 16, 16)
    x, m1 = (dev(a) for a in synth.synth_noise(shape, 2, seed=63))
    mo = dev(synth.synth_model_output(shape, True, 64))
    nan = torch.full_like(x, float("nan"))
    flags = d._flags(True)
    a = step(d, mo, x, None, None, None, [5], flags, 1, False)
    b = step(d, mo, x, nan, nan, None, [5], flags, 1, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = step(d, mo, x, m1, nan, None, [5], flags, 2, False)
    assert torch.isfinite(c[0]).all() and not torch.equal(c[0], a[0])


def test_out_of_range_t_gives_nan_for_that_sample_only():
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="logsnr10")
    shape = (2, 1, 4, 8, 8)
    x, m1, m2, z = (dev(a) for a in synth.synth_noise(shape, 4, seed=65))
    mo = dev(synth.synth_model_output(shape, True, 66))
    flags = d._flags(True)
    for bad in (10, -1, 1 << 40):
        good = step(d, mo[:1], x[:1], m1[:1], m2[:1], z[:1], [3], flags, 2, True)
        s, x0 = step(d, mo, x, m1, m2, z, [3, bad], flags, 2, True)
        assert torch.equal(s[:1], good[0]) and torch.equal(x0[:1], good[1])
        assert torch.isnan(s[1]).all() and torch.isnan(x0[1]).all()


# -------------------------------------------------------------------- loop
@pytest.mark.parametrize("resp", ["ddim10", "logsnr10"])
def test_order_one_loop_is_ddim(resp):
    """ODE order 1 against ddim_sample_loop(eta=0) and SDE order 1 against eta=1 with the same step noise, on the
    tiny SR network's engine path.

    Step by step on DDIM's own inputs (its x_k and the network's output on it), one solver launch gives the DDIM
    step's pred_xstart bitwise and its sample within 1e-5 (max-norm relative): the two forms differ only in fp32 rounding.
    Chained over the loop, every step's sample and pred_xstart stay within 2e-4.  The chained bar is wider because
    pred_xstart = sqrt_recip_acp x - sqrt_recipm1_acp eps multiplies the step input's ~1e-7 rounding difference by
    25-60 at the noisy steps, and the network carries it on.  Measured on an MI355X (f16x3): one step <= 3.2e-6;
    chained, the sample <= 4.2e-5 and pred_xstart <= 1.4e-4 (step 1 of "logsnr10", eta = 1); the first step, whose
    input is shared, 1.5e-7 and pred_xstart bitwise."""
    model, diff = build(TINY, resp)
    shape = (2, 1, 8, 16, 16)
    T = diff.num_timesteps
    draws = [dev(a) for a in synth.synth_noise(shape, T + 1, seed=10)]
    lr = dev(synth.synth_low_res(shape, seed=1234))
    kw = {"low_res": lr}
    for eta, stochastic in ((0.0, False), (1.0, True)):
        a = list(diff.ddim_sample_loop_progressive(model, shape, draws[0], model_kwargs=kw, eta=eta,
                                                   step_noise=draws[1:]))
        b = list(diff.dpm_solver_sample_loop_progressive(model, shape, draws[0], model_kwargs=kw, order=1,
                                                         stochastic=stochastic, step_noise=draws[1:]))
        assert len(a) == len(b) == T
        flags = diff._flags(True)
        x, single = draws[0], []
        for k, ref in enumerate(a):
            t = torch.full((shape[0],), T - 1 - k, dtype=torch.int64, device="cuda")
            with torch.no_grad():
                out = model(x, diff._model_timesteps(t), low_res=lr)
            z = draws[1 + k]
            ddim = diff._update("ddim", out, x, t, z, True, eta)
            one = diff._solver_step(out, x, None, None, z if stochastic else None, t, flags, 1, stochastic, 1)
            assert torch.equal(one["pred_xstart"], ddim["pred_xstart"]), k
            single.append(rel_err(np_(one["sample"]), np_(ddim["sample"])))
            x = ref["sample"]
        chained = [(rel_err(np_(q["sample"]), np_(p["sample"])), rel_err(np_(q["pred_xstart"]), np_(p["pred_xstart"])))
                   for p, q in zip(a, b)]
        print("%s eta=%g: one step %.2e; chained sample %s; pred_xstart %s"
              % (resp, eta, max(single), " ".join("%.1e" % e[0] for e in chained),
                 " ".join("%.1e" % e[1] for e in chained)))
        assert max(single) < 1e-5, single
        assert max(max(e) for e in chained) < 2e-4, chained


def _oracle_solver(diff, sd, cfg, x, lr, order, stochastic, draws, clip=True):
    """The CPU oracle network and an fp64 numpy solver on the fp64 weights: each step's sample."""
    from oracle import unet_ref
    tab = diff.dpm_solver_coefficients(order, stochastic)
    T = diff.num_timesteps
    C = x.shape[1]
    xs, hist, out = x.astype(np.float64), [], []
    for k in range(T):
        s = T - 1 - k
        with torch.no_grad():
            mo = unet_ref.unet_forward(sd, cfg, torch.from_numpy(xs.astype(np.float32)),
                                       torch.tensor([diff.timestep_map[s]] * x.shape[0]), lr).numpy()
        eps = mo[:, :C].astype(np.float64)
        x0 = diff.sqrt_recip_alphas_cumprod[s] * xs - diff.sqrt_recipm1_alphas_cumprod[s] * eps
        if clip:
            x0 = np.clip(x0, -1, 1)
        w = tab[s]
        nxt = w[0] * xs + w[1] * x0
        if hist:
            nxt = nxt + w[2] * hist[0]
        if len(hist) > 1:
            nxt = nxt + w[3] * hist[1]
        if stochastic:
            nxt = nxt + w[4] * draws[k].astype(np.float64)
        hist = [x0] + hist[:1]
        xs = nxt
        out.append(xs)
    return out


@pytest.mark.parametrize("order,stochastic", [(2, False), (3, False), (2, True)])
def test_higher_orders_vs_cpu_oracle(order, stochastic):
    """Orders 2 and 3 (and the SDE form at 2) on "logsnr10" against oracle/unet_ref.py plus an fp64 solver: every
    step within the sampler loops' 1e-3 bar."""
    from oracle import unet_ref
    model, diff = build(TINY, "logsnr10", precision="f32")
    shape = (1, 1, 4, 16, 16)
    T = diff.num_timesteps
    draws = synth.synth_noise(shape, T + 1, seed=12)
    lr = synth.synth_low_res(shape, seed=1234)
    got = list(diff.dpm_solver_sample_loop_progressive(model, shape, dev(draws[0]), model_kwargs={"low_res": dev(lr)},
                                                       order=order, stochastic=stochastic,
                                                       step_noise=[dev(a) for a in draws[1:]]))
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = _oracle_solver(diff, sd, unet_ref.sr_config(**TINY), draws[0], torch.from_numpy(lr), order, stochastic,
                         draws[1:])
    errs = [rel_err(np_(g["sample"]), r) for g, r in zip(got, ref)]
    print("order %d stochastic %s: per step %s" % (order, stochastic, " ".join("%.1e" % e for e in errs)))
    assert max(errs) < 1e-3, errs


class GaussianEps(torch.nn.Module):
    """The exact eps predictor of data x0 ~ N(MU, SD^2) under the base schedule, conditioned on the original
    timestep the diffusion maps each step to."""

    def __init__(self, base_acp):
        super().__init__()
        self.register_buffer("acp", torch.from_numpy(np.asarray(base_acp, dtype=np.float64)))

    def forward(self, x, t):
        acp = self.acp[t.long()].reshape((-1,) + (1,) * (x.dim() - 1))
        a, sig2 = acp.sqrt(), 1 - acp
        return (sig2.sqrt() * (x.double() - a * MU) / (acp * SD ** 2 + sig2)).float()


def test_analytic_gaussian_model_converges():
    """The loop's non-engine path on the exact eps model of Gaussian data, in fp32 on the device: its error against
    the exact solution falls from 50 to 100 log-SNR steps as the CPU test's fp64 run does (>= 1.8x / 3.0x / 4.0x
    for orders 1 / 2 / 3), and its final samples agree with that fp64 run."""
    from guided_diffusion import gaussian_diffusion as gd
    base = np.cumprod(1.0 - gd.get_named_beta_schedule("linear", 1000))
    model = GaussianEps(base).cuda()
    shape = (1, 1, 16, 32, 32)
    xT = synth.synth_noise(shape, 1, seed=70)[0]
    err, gap = {}, {}
    for n in (50, 100):
        d = su.create_gaussian_diffusion(steps=1000, timestep_respacing="logsnr%d" % n)
        exact = gaussian_exact(d, xT.astype(np.float64))
        for order in (1, 2, 3):
            got = np_(d.dpm_solver_sample_loop(model, shape, dev(xT), clip_denoised=False, device="cuda",
                                                  order=order))
            err[n, order] = float(np.abs(got - exact).max())
            gap[n, order] = float(np.abs(got - solve_gaussian(d, order, xT.astype(np.float64))).max())
    print("errors", err, "gap to fp64", gap)
    for order, ratio in ((1, 1.8), (2, 3.0), (3, 4.0)):
        assert err[50, order] / err[100, order] >= ratio, (order, err)
    assert max(gap.values()) < 1e-4, gap


def test_engine_paths_and_repeatability():
    """Order 2 on the tiny SR network: eager, step-graph and native-plan loops are bitwise equal and repeatable;
    the yielded dicts keep their values while the loop runs on."""
    model, diff = build(TINY, "logsnr10")
    shape = (2, 1, 8, 16, 16)
    noise = dev(synth.synth_noise(shape, 1, seed=10)[0])
    kw = {"low_res": dev(synth.synth_low_res(shape, seed=1234))}

    def run():
        steps = list(diff.dpm_solver_sample_loop_progressive(model, shape, noise.clone(), model_kwargs=kw, order=2))
        return [s["sample"].clone() for s in steps], steps

    eager, held = run()
    for a, s in zip(eager, held):
        assert torch.equal(a, s["sample"])
    assert torch.equal(eager[-1], held[-1]["pred_xstart"]) and torch.isfinite(eager[-1]).all()
    assert all(torch.equal(a, b) for a, b in zip(eager, run()[0]))
    try:
        model.step_graph = True
        graph = run()[0]
        eng = model.engine()
        assert eng.step_graph and any(pl.graphs for pl in eng.plans.values())
        model.step_graph = False
        model.native_plan = True
        native = run()[0]
        assert model.engine().native_plan and model.engine().native_plans
    finally:
        model.step_graph = model.native_plan = False
    for other in (graph, native):
        assert all(torch.equal(a, b) for a, b in zip(eager, other))


def test_two_dimensional_network_at_order_two():
    """create_model_and_diffusion's 2-D RGB network through _call_model: (N, 3, H, W), voxels spanning the channels,
    the eps half of a 6-channel output."""
    fl = su.model_and_diffusion_defaults()
    fl.update(image_size=64, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", num_head_channels=32,
              attention_resolutions="16", learn_sigma=True, use_scale_shift_norm=True, timestep_respacing="logsnr6")
    model, diff = su.create_model_and_diffusion(**fl)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape), 2))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    shape = (2, 3, 32, 48)
    noise = dev(synth.synth_noise(shape, 1, seed=3)[0])
    steps = list(diff.dpm_solver_sample_loop_progressive(model, shape, noise, order=2))
    assert len(steps) == 6
    for s in steps:
        assert s["sample"].shape == shape and torch.isfinite(s["sample"]).all()
    assert torch.equal(steps[-1]["sample"], steps[-1]["pred_xstart"])
    again = diff.dpm_solver_sample_loop(model, shape, noise, order=2)
    assert torch.equal(again, steps[-1]["sample"])


def test_published_64_properties():
    """The published network at 1 x 64^3, "logsnr10", order 2: every step finite, the last sample is its
    pred_xstart, and the progressive form's step k is exactly one network call plus one solver launch on step
    k - 1's sample and history (k = 0, 1, 5, 9); the step graph gives the eager bits."""
    model, diff = build(PUBLISHED, "logsnr10")
    T = diff.num_timesteps
    shape = (1, 1, 64, 64, 64)
    noise = dev(synth.synth_noise(shape, 1, seed=10)[0])
    lr = dev(synth.synth_low_res(shape, seed=1234))
    kw = {"low_res": lr}
    flags = diff._flags(True)
    prev, hist, checked = noise, [], 0
    for k, r in enumerate(diff.dpm_solver_sample_loop_progressive(model, shape, noise, model_kwargs=kw, order=2)):
        assert torch.isfinite(r["sample"]).all() and torch.isfinite(r["pred_xstart"]).all(), k
        if k in (0, 1, 5, 9):
            s = T - 1 - k
            t = torch.tensor([s], device="cuda")
            with torch.no_grad():
                out = model(prev, diff._model_timesteps(t), low_res=lr)
            p = 1 if s == 0 else min(2, k + 1)
            one = diff._solver_step(out, prev, hist[0] if p >= 2 else None, None, None, t, flags, 2, False, p)
            assert torch.equal(one["sample"], r["sample"]) and torch.equal(one["pred_xstart"], r["pred_xstart"]), k
            checked += 1
        prev, hist = r["sample"], [r["pred_xstart"]] + hist[:1]
    assert checked == 4 and torch.equal(prev, hist[0])
    try:
        model.step_graph = True
        g = diff.dpm_solver_sample_loop(model, shape, noise, model_kwargs=kw, order=2)
    finally:
        model.step_graph = False
    assert torch.equal(g, prev)


# ------------------------------------------------------------------ script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry_dpm", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inference_script_with_dpm_solver(tmp_path):
    vol = np.random.default_rng(5).random((20, 24, 24), dtype=np.float32)
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    mod = _script()

    def run(tag, *extra):
        path = mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / tag)] + list(extra))
        assert path == str(tmp_path / tag / "denoised_pet.npz") and os.path.exists(path)
        return np.load(path)["arr_0"]

    ddim = run("ddim", "--timestep_respacing", "ddim10", "--use_ddim", "True")
    dpm1 = run("dpm1", "--timestep_respacing", "ddim10", "--use_dpm_solver", "True", "--solver_order", "1",
               "--use_ddim", "True")
    assert np.isfinite(ddim).all() and np.abs(ddim).max() > 0
    # measured on an MI355X: 2.9e-5 (the chained drift of test_order_one_loop_is_ddim)
    assert rel_err(dpm1, ddim) < 1e-4, rel_err(dpm1, ddim)
    dpm2 = run("dpm2", "--timestep_respacing", "logsnr10", "--use_dpm_solver", "True", "--solver_order", "2")
    assert dpm2.shape == (24, 24, 20) and dpm2.dtype == np.float32 and np.isfinite(dpm2).all()
    sde = run("sde", "--timestep_respacing", "logsnr10", "--use_dpm_solver", "True", "--solver_stochastic", "True",
              "--batch_size", "4")
    assert np.isfinite(sde).all() and not np.array_equal(sde, dpm2)
    assert math.isfinite(float(np.abs(sde).max()))
