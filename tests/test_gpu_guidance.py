"""
The low-pass data-consistency pull on the GPU: ddpm3d_xstart_pull against a composition of existing
entries (bitwise) and against fp64 (the bound of include/ddpm3d.h), its containment, the three *_step_x0 entries
against the existing step entries (bitwise), the guided p_sample / ddim_sample against the reference's denoised_fn path
(tests/golden/guidance.npz), and every loop with guide= against its own step-by-step composition (bitwise).
"""

import numpy as np
import pytest
import torch

import guidance_ref as gr
from conftest import rel_err
from guided_diffusion import _hip as H
from guided_diffusion import gaussian_diffusion as gd
from guided_diffusion import guidance, joint, metrics, patches, synth
from guided_diffusion import script_util as su

pytestmark = pytest.mark.gpu

VARIANTS = {"learned_range": dict(learn_sigma=True), "fixed_large": dict(learn_sigma=False),
            "fixed_small": dict(learn_sigma=False, sigma_small=True),
            "xstart": dict(learn_sigma=True, predict_xstart=True)}
# (N, D, H, W), radii along (D, H, W): one voxel; a radius above the extent; W no multiple of 4 or 64 and more than one
# workgroup per sample; the pointwise pull; one and two skipped passes
SHAPES = [((1, 1, 1, 1), (1, 1, 1)), ((2, 3, 5, 70), (4, 2, 1)), ((3, 7, 9, 65), (1, 2, 3)),
          ((2, 16, 16, 16), (0, 0, 0)), ((2, 5, 6, 7), (2, 0, 1)), ((3, 4, 9, 5), (0, 3, 0)), ((1, 6, 3, 4), (16, 0, 0))]
WEIGHTS = (0.0, 0.37, 1.0)


def np_(t):
    return t.detach().cpu().numpy()


def diffusion(variant, resp="250"):
    return su.create_gaussian_diffusion(steps=1000, timestep_respacing=resp, **VARIANTS[variant])


def pull_with(radii, weight=1.0, stop_t=0, measurement=None):
    """a LowPassPull on guidance_ref.taps_for's tables (the tests choose radii, not millimetres)"""
    p = guidance.LowPassPull(0, None, weight=weight, stop_t=stop_t, measurement=measurement)
    taps = [[float(v) for v in t] for t in gr.taps_for(radii)]
    p.taps = metrics.GaussianTaps((0.0,) * 3, None, (0.0,) * 3, tuple(radii), taps)
    return p


def inputs(shape4, variant, seed=0):
    N, D, Hh, W = shape4
    shape = (N, 1, D, Hh, W)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=100 + seed)[0]).cuda()
    y = torch.from_numpy(synth.synth_low_res(shape, seed=200 + seed)).cuda() * 2 - 1
    mo = torch.from_numpy(synth.synth_model_output(shape, VARIANTS[variant]["learn_sigma"], 300 + seed)).cuda()
    return x, y, mo


def steps_t(d, N):
    T = d.num_timesteps
    return torch.tensor([0, T // 2, T - 1][:N] if N <= 3 else [T - 1] * N, device="cuda")


def raw_x0(d, mo, x, t):
    return d.p_mean_variance(lambda *a, **k: mo, x, t, clip_denoised=False)["pred_xstart"]


def composed(d, mo, x, y, t, pull, clip):
    """the pull from existing entries: p_mean_variance's unclipped pred_xstart, a torch subtraction,
    metrics.gaussian_smooth per sample, torch.mul, torch.add, clamp"""
    x0 = raw_x0(d, mo, x, t)
    res = y - x0
    g = torch.stack([metrics.gaussian_smooth(res[n, 0].contiguous(), pull.taps)[None] for n in range(x.shape[0])])
    out = torch.add(x0, torch.mul(g, pull.weight))
    return out.clamp(-1, 1) if clip else out


@pytest.mark.parametrize("variant", ["learned_range", "fixed_large", "xstart"])
@pytest.mark.parametrize("shape4, radii", SHAPES)
def test_pull_equals_a_composition_of_existing_entries_bitwise(shape4, radii, variant):
    d = diffusion(variant)
    x, y, mo = inputs(shape4, variant)
    t = steps_t(d, shape4[0])
    for clip in (True, False):
        flags = d._flags(clip)
        for w in WEIGHTS:
            pull = pull_with(radii, weight=w)
            got = pull.apply(mo, x, t, flags, d, measurement=y)
            want = composed(d, mo, x, y, t, pull, clip)
            assert got.shape == x.shape and torch.isfinite(got).all()
            assert torch.equal(got, want), (clip, w, float((got - want).abs().max()))
            if w == 0.0:      # clamp(x0_raw), as numbers
                x0 = raw_x0(d, mo, x, t)
                assert np.array_equal(np_(got), np_(x0.clamp(-1, 1) if clip else x0))


@pytest.mark.parametrize("variant", ["learned_range", "xstart"])
@pytest.mark.parametrize("shape4, radii", SHAPES)
def test_pull_within_its_bound_of_fp64(shape4, radii, variant):
    """Every voxel within u |x0_raw + w m| + w ((1 + u)^3 prod (1 + c_a u) - 1) M of the fp64 operator on the same fp32
    x0_raw, y, taps and w (include/ddpm3d.h), with and without the clip.  Measured on an MI355X, largest fraction of
    the bound used: 0.91 (the pointwise pull, whose bound is three roundings of the residual plus one of the result);
    0.22 to 0.43 with one to three passes; 0.04 on a single voxel."""
    d = diffusion(variant)
    x, y, mo = inputs(shape4, variant, seed=1)
    t = steps_t(d, shape4[0])
    x0 = np_(raw_x0(d, mo, x, t))
    worst = 0.0
    for w in (0.37, 1.0):
        pull = pull_with(radii, weight=w)
        exact, bound = gr.pull64(x0, np_(y), gr.taps_for(radii), pull.weight)
        for clip in (True, False):
            got = np_(pull.apply(mo, x, t, d._flags(clip), d, measurement=y)).astype(np.float64)
            err = np.abs(got - (np.clip(exact, -1, 1) if clip else exact))
            assert (err <= bound).all(), (w, clip, float((err / bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("pull vs fp64 %s %s %s: largest fraction of the bound %.3f" % (shape4, radii, variant, worst))


def test_pull_containment_and_repeatability():
    """a NaN planted in sample 1 (in x, the measurement and the model output) leaves samples 0 and 2 bit-identical; an
    out-of-range t gives NaN for that sample only; two runs give equal bits"""
    d = diffusion("learned_range")
    shape4, radii = (3, 7, 9, 65), (2, 3, 4)
    x, y, mo = inputs(shape4, "learned_range", seed=2)
    t = steps_t(d, 3)
    pull = pull_with(radii, weight=0.8)
    flags = d._flags(True)
    a = pull.apply(mo, x, t, flags, d, measurement=y)
    assert torch.equal(a, pull.apply(mo, x, t, flags, d, measurement=y))
    for which in range(3):
        xs, ys, ms = x.clone(), y.clone(), mo.clone()
        (xs, ys, ms)[which][1, 0, 3, 4, 5] = float("nan")
        b = pull.apply(ms, xs, t, flags, d, measurement=ys)
        assert torch.equal(b[0], a[0]) and torch.equal(b[2], a[2]), which
    yn = y.clone()
    yn[1, 0, 3, 4, 5] = float("nan")
    nc = pull.apply(mo, x, t, d._flags(False), d, measurement=yn)
    assert torch.isnan(nc[1]).any() and torch.isfinite(nc[0]).all() and torch.isfinite(nc[2]).all()
    T = d.num_timesteps
    bad = pull.apply(mo, x, torch.tensor([int(t[0]), T, -1], device="cuda"), flags, d, measurement=y)
    assert torch.equal(bad[0], a[0]) and torch.isnan(bad[1]).all() and torch.isnan(bad[2]).all()
    # the pointwise form answers an out-of-range t the same way
    p0 = pull_with((0, 0, 0))
    bad0 = p0.apply(mo, x, torch.tensor([T + 5, 1, 2], device="cuda"), flags, d, measurement=y)
    assert torch.isnan(bad0[0]).all() and torch.isfinite(bad0[1:]).all()


@pytest.mark.parametrize("radii", [(0, 0, 0), (1, 2, 3)])
def test_pull_keeps_nan_through_the_clip(radii):
    """A NaN in the model output (a diverged network) stays NaN through the pull's clip, as through x.clamp(-1, 1):
    the pull equals its composition of existing entries, whose clip is torch's, NaN for NaN and bit for bit elsewhere.
    The pointwise pull is NaN at exactly the planted voxels; a smoothing pull spreads them and leaves the rest finite."""
    d = diffusion("learned_range")
    shape4 = (3, 7, 9, 65)
    x, y, mo = inputs(shape4, "learned_range", seed=3)
    t = steps_t(d, 3)
    planted = [(0, 0, 0, 0, 0), (1, 0, 3, 4, 5), (2, 0, 6, 8, 64)]
    for p in planted:
        mo[p] = float("nan")
    pull = pull_with(radii, weight=0.8)
    got = pull.apply(mo, x, t, d._flags(True), d, measurement=y)
    want = composed(d, mo, x, y, t, pull, True)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
    assert all(bool(torch.isnan(got[p])) for p in planted)
    count = int(torch.isnan(got).sum())
    assert count == 3 if radii == (0, 0, 0) else 3 < count < got.numel() // 2
    assert float(got.nan_to_num(0.0).abs().max()) <= 1.0
    if radii == (0, 0, 0):               # the CPU reference's clip keeps them too
        ref = gr.pulled_x0(d.coef_table(), mo.cpu(), x.cpu(), t.cpu(), y.cpu(), gr.taps_for(radii), pull.weight,
                           False, True)
        assert np.array_equal(np.isnan(ref.numpy()), np_(torch.isnan(got)))


# ------------------------------------------------------------------------------------------- the *_step_x0 entries
def _key(N, seed=7):
    return gd.NoiseKey(seed, list(range(11, 11 + N)))


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("learn", [True, False])
def test_step_x0_entries_equal_the_predict_xstart_entries_bitwise(learn, clip):
    """each *_step_x0 entry fed an arbitrary xstart == the existing entry under F_PREDICT_XSTART with the model output's
    first half replaced by that xstart; the keyed form == the un-keyed form fed ddpm3d_noise_fill's output"""
    eps = su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", learn_sigma=learn)
    xst = su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", learn_sigma=learn, predict_xstart=True)
    shape = (3, 1, 5, 6, 67)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=61)[0]).cuda()
    mo = torch.from_numpy(synth.synth_model_output(shape, learn, 62)).cuda()
    xs = (torch.from_numpy(synth.synth_noise(shape, 1, seed=63)[0]) * 0.8).cuda()      # some beyond the clip
    z = torch.from_numpy(synth.synth_noise(shape, 1, seed=64)[0]).cuda()
    m1, m2 = (torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 2, seed=65))
    swapped = mo.clone()
    swapped[:, :1] = xs
    t = steps_t(eps, 3)
    key = _key(3)
    zk = key.fill(4, shape)

    def same(a, b, what):
        assert torch.equal(a["sample"], b["sample"]) and torch.equal(a["pred_xstart"], b["pred_xstart"]), what
        assert torch.equal(a["pred_xstart"], xs.clamp(-1, 1) if clip else xs), what

    for kind, eta in (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)):
        a = eps._update(kind, mo, x, t, z, clip, eta, xstart=xs)
        same(a, xst._update(kind, swapped, x, t, z, clip, eta), (kind, eta))
        k = eps._update(kind, mo, x, t, None, clip, eta, noise_key=key, draw=4, xstart=xs)
        same(k, xst._update(kind, swapped, x, t, None, clip, eta, noise_key=key, draw=4), (kind, eta, "keyed"))
        same(k, eps._update(kind, mo, x, t, zk, clip, eta, xstart=xs), (kind, eta, "keyed vs filled"))
    flags_e, flags_x = eps._flags(clip), xst._flags(clip)
    for order in (1, 2, 3):
        for stochastic in (False, True):
            if stochastic and order == 3:
                continue
            zz = z if stochastic else None
            a = eps._solver_step(mo, x, m1, m2, zz, t, flags_e, order, stochastic, order, xstart=xs)
            same(a, xst._solver_step(swapped, x, m1, m2, zz, t, flags_x, order, stochastic, order), (order, stochastic))
            if stochastic:
                k = eps._solver_step(mo, x, m1, m2, None, t, flags_e, order, True, order, key, 4, xstart=xs)
                same(k, xst._solver_step(swapped, x, m1, m2, None, t, flags_x, order, True, order, key, 4),
                     (order, "keyed"))
                same(k, eps._solver_step(mo, x, m1, m2, zk, t, flags_e, order, True, order, xstart=xs),
                     (order, "keyed vs filled"))


# ------------------------------------------------------------------------------------ against the reference's path
G_SEEDS = dict(x=22, model_output=23, measurement=77, noise=78)        # make_golden_guidance.SEEDS
G_SHAPE = (3, 1, 4, 16, 16)
G_RADII = {"r123": (1, 2, 3), "r000": (0, 0, 0)}


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("rtag", sorted(G_RADII))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_guided_steps_vs_reference(golden, variant, rtag, clip):
    """p_sample and ddim_sample (eta 0 and 0.5) with guide= against the reference's own calls with the pull as
    denoised_fn: pred_xstart and every sample within 1e-5 (max-norm relative), the bar of the un-guided entries
    (tests/test_gpu_ddim_reverse.py).  Measured on an MI355X, all sixteen cases: pred_xstart and the three DDIM samples
    bitwise (0.0); p_sample bitwise under the fixed variances and 6.3e-8 to 6.5e-8 under the learned one (expf within
    an ulp of the reference host's exp)."""
    g = golden("guidance.npz")
    key = "%s/%s/%s" % (variant, rtag, "clip" if clip else "noclip")
    d = diffusion(variant)
    learn = VARIANTS[variant]["learn_sigma"]
    x = torch.from_numpy(synth.synth_noise(G_SHAPE, 1, seed=G_SEEDS["x"])[0]).cuda()
    y = torch.from_numpy(synth.synth_low_res(G_SHAPE, seed=G_SEEDS["measurement"])).cuda()
    z = torch.from_numpy(synth.synth_noise(G_SHAPE, 1, seed=G_SEEDS["noise"])[0]).cuda()
    mo = torch.from_numpy(synth.synth_model_output(G_SHAPE, learn, G_SEEDS["model_output"])).cuda()
    t = torch.from_numpy(g["t"])
    calls = []

    def model(xx, tt, **kw):
        calls.append(1)
        return mo

    pull = pull_with(G_RADII[rtag], weight=float(g["weight"]), measurement=y)
    p = d.p_sample(model, x, t, clip_denoised=clip, noise=z, guide=pull)
    errs = {"pred_xstart": rel_err(np_(p["pred_xstart"]), g[key + "/pred_xstart"]),
            "p_sample": rel_err(np_(p["sample"]), g[key + "/p_sample"])}
    for eta in (0.0, 0.5):
        r = d.ddim_sample(model, x, t, clip_denoised=clip, eta=eta, noise=z, guide=pull)
        assert torch.equal(r["pred_xstart"], p["pred_xstart"])
        errs["ddim_eta%g" % eta] = rel_err(np_(r["sample"]), g[key + "/ddim_eta%g" % eta])
    assert len(calls) == 3
    # low_res in model_kwargs takes the measurement's place
    q = d.p_sample(model, x, t, clip_denoised=clip, noise=z, model_kwargs={"low_res": y},
                   guide=pull_with(G_RADII[rtag], weight=float(g["weight"])))
    assert torch.equal(q["sample"], p["sample"])
    print(key, " ".join("%s %.2e" % kv for kv in sorted(errs.items())))
    assert max(errs.values()) < 1e-5, errs


# ---------------------------------------------------------------------------------------------------------- the loops
TINY = dict(large_size=16, small_size=16, num_channels=32, num_res_blocks=1, num_head_channels=64,
            attention_resolutions="1000", learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True,
            timestep_respacing="3")
SHAPE = (2, 1, 16, 16, 16)


@pytest.fixture(scope="module")
def tiny():
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(TINY)
    model, diff = su.sr_create_model_and_diffusion(**fl)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape)))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(SHAPE, 4, seed=10)]
    low = torch.from_numpy(synth.synth_low_res(SHAPE, seed=1234)).cuda()
    return model, diff, draws, low


LOOPS = {"ddpm": ("p_sample_loop", {}), "ddim": ("ddim_sample_loop", dict(eta=0.5)),
         "dpm_ode": ("dpm_solver_sample_loop", dict(order=3)),
         "dpm_sde": ("dpm_solver_sample_loop", dict(order=2, stochastic=True))}


def compose(diff, model, low, pull, kind, start, step_noise=None, key=None, trace=None, clip=True):
    """a guided loop written out: a network call, pull.apply, then the *_step_x0 step -> the per-step dicts"""
    kw = LOOPS[kind][1]
    T = diff.num_timesteps
    flags = diff._flags(clip)
    img, hist, outs = start, [], []
    with torch.no_grad():
        for k, i in enumerate(range(T - 1, -1, -1)):
            t = torch.full((img.shape[0],), i, device="cuda", dtype=torch.int64)
            mo = diff._call_model(model, img, t, {"low_res": low})
            xs = pull.apply(mo, img, t, flags, diff, measurement=low) if pull.active(diff, i) else None
            if kind in ("ddpm", "ddim"):
                z = None if key is not None else step_noise[k]
                res = diff._update(kind, mo, img, t, z, clip, kw.get("eta", 0.0), noise_key=key, draw=k + 1, xstart=xs)
            else:
                sde = kw.get("stochastic", False)
                p = 1 if i == 0 else min(kw["order"], k + 1)
                z = step_noise[k] if sde and key is None else None
                res = diff._solver_step(mo, img, hist[0] if p >= 2 else None, hist[1] if p >= 3 else None, z, t,
                                        flags, kw["order"], sde, p, key if sde else None, k + 1, xstart=xs)
            if trace is not None:
                trace.add(res["pred_xstart"], hist[0] if hist else None, diff.timestep_map[i], T)
            if xs is not None:
                assert torch.equal(res["pred_xstart"], xs.clamp(-1, 1) if clip else xs)
            outs.append(res)
            img = res["sample"]
            hist = [res["pred_xstart"]] + hist[:1]
    return outs


@pytest.mark.parametrize("kind", sorted(LOOPS))
def test_guided_loops_equal_their_composition_bitwise(tiny, kind):
    """every loop with guide= == network call, pull.apply, *_step_x0 step, bit for bit: with injected noise, with
    noise_key=, with trace= (whose rows are the pulled pred_xstart's) and with a stop_t between two steps; a stop_t
    above the first timestep and a weight of 0 are the un-guided loop"""
    model, diff, draws, low = tiny
    name, kw = LOOPS[kind]
    mk = {"low_res": low}
    tmap = list(diff.timestep_map)
    assert diff.num_timesteps == 3
    noisy = kind != "dpm_ode"
    sn = dict(step_noise=draws[1:]) if noisy else {}
    for stop in (tmap[1], 0):
        pull = pull_with((2, 1, 3), weight=0.6, stop_t=stop)
        steps = list(getattr(diff, name + "_progressive")(model, SHAPE, noise=draws[0], model_kwargs=mk, guide=pull,
                                                          **sn, **kw))
        want = compose(diff, model, low, pull, kind, draws[0], draws[1:])
        for s, w in zip(steps, want):
            assert torch.equal(s["sample"], w["sample"]) and torch.equal(s["pred_xstart"], w["pred_xstart"]), stop
    final = getattr(diff, name)(model, SHAPE, noise=draws[0], model_kwargs=mk, guide=pull, **sn, **kw)
    assert torch.equal(final, want[-1]["sample"])
    plain = getattr(diff, name)(model, SHAPE, noise=draws[0], model_kwargs=mk, **sn, **kw)
    assert not torch.equal(final, plain)
    for off in (pull_with((2, 1, 3), weight=0.6, stop_t=tmap[-1] + 1), pull_with((2, 1, 3), weight=0.0)):
        assert torch.equal(getattr(diff, name)(model, SHAPE, noise=draws[0], model_kwargs=mk, guide=off, **sn, **kw),
                           plain)
    # the pull's own measurement instead of low_res
    own = pull_with((2, 1, 3), weight=0.6, measurement=low)
    assert torch.equal(getattr(diff, name)(model, SHAPE, noise=draws[0], model_kwargs=mk, guide=own, **sn, **kw), final)
    # keyed noise
    key = _key(SHAPE[0])
    keyed = list(getattr(diff, name + "_progressive")(model, SHAPE, model_kwargs=mk, guide=pull, noise_key=key, **kw))
    want = compose(diff, model, low, pull, kind, key.fill(0, SHAPE), key=key)
    for s, w in zip(keyed, want):
        assert torch.equal(s["sample"], w["sample"]) and torch.equal(s["pred_xstart"], w["pred_xstart"])
    # trace: the rows are those of the pulled pred_xstart's, and tracing changes nothing
    target = torch.from_numpy(synth.synth_x_start(SHAPE, 5)).cuda()
    tr, tr_want = metrics.StepTrace(target=target), metrics.StepTrace(target=target)
    traced = getattr(diff, name)(model, SHAPE, noise=draws[0], model_kwargs=mk, guide=pull, trace=tr, **sn, **kw)
    want = compose(diff, model, low, pull, kind, draws[0], draws[1:], trace=tr_want)
    assert torch.equal(traced, final) and torch.equal(traced, want[-1]["sample"])
    assert np.array_equal(tr.records(), tr_want.records()) and tr.t == tr_want.t
    last = metrics.StepTrace(target=target)
    last.add(want[-1]["pred_xstart"], want[-2]["pred_xstart"], tmap[0], 3)
    assert np.array_equal(tr.records()[-1], last.records()[0])


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_guided_joint_loop_equals_its_composition_bitwise(tiny, kind):
    """the joint loop pulls every patch towards its own conditioning patch: == gather, network call, pull.apply on the
    gathered conditioning, *_step_x0 step, blend, bit for bit (one batch of all patches)"""
    model, diff, _, _ = tiny
    vol = synth.synth_low_res((10, 40, 16), seed=77)
    geom = patches.joint_geometry(vol.shape, 16)
    P = geom.n_patches
    cshape = (1,) + tuple(geom.canvas)
    zs = [torch.from_numpy(a).cuda() for a in synth.synth_noise(cshape, 4, seed=12)]
    pull = pull_with((1, 2, 2), weight=0.7)
    eta = 0.5 if kind == "ddim" else 0.0
    steps = list(joint.sample_loop_progressive(diff, model, vol, geom, kind=kind, batch_size=P, noise=zs[0],
                                               step_noise=zs[1:], eta=eta, guide=pull))
    lr = joint.gather(joint._canvas_of(vol, geom, torch.device("cuda", torch.cuda.current_device())), geom)
    img = zs[0]
    flags = diff._flags(True)
    with torch.no_grad():
        for k, i in enumerate(range(diff.num_timesteps - 1, -1, -1)):
            x = joint.gather(img, geom)
            t = torch.full((P,), i, device="cuda", dtype=torch.int64)
            mo = diff._call_model(model, x, t, {"low_res": lr})
            xs = pull.apply(mo, x, t, flags, diff, measurement=lr)
            res = diff._update(kind, mo, x, t, joint.gather(zs[k + 1], geom), True, eta, xstart=xs)
            img = joint.blend(res["sample"], geom)
            assert torch.equal(steps[k]["sample"], img), k
            assert torch.equal(steps[k]["pred_xstart"], joint.blend(res["pred_xstart"], geom)), k
    plain = joint.sample_loop(diff, model, vol, geom, kind=kind, batch_size=P, noise=zs[0], step_noise=zs[1:], eta=eta)
    assert not torch.equal(plain, img)
    off = joint.sample_loop(diff, model, vol, geom, kind=kind, batch_size=P, noise=zs[0], step_noise=zs[1:], eta=eta,
                            guide=pull_with((1, 2, 2), weight=0.0))
    assert torch.equal(off, plain)
