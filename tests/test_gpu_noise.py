"""
Keyed sampler noise on the GPU: the generator's words against the numpy reference exactly, the
normals against the fp64 reference within the derived bound, the invariances that make a keyed run independent of the
batch and of the launch, every keyed step entry bit for bit against its un-keyed entry fed with ddpm3d_noise_fill's
output (plain and with a canvas geometry), and every loop with noise_key= against the same loop on explicit tensors.
"""

import numpy as np
import pytest
import torch

import noise_ref as NR
from guided_diffusion import _hip as H
from guided_diffusion import dist_util, joint, patches
from guided_diffusion import script_util as su
from guided_diffusion import synth
from guided_diffusion.gaussian_diffusion import NoiseKey

pytestmark = pytest.mark.gpu

PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True,
                 use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)

# odd sizes misalign rows 1 and 2 for the four-wide fill; 262147 > 1024 workgroups x 256 turns the per-voxel kernels'
# grid-stride loop over, 1048583 > 1024 x 256 counters that of the fill's one-counter-per-thread form
VOXELS = [1, 2, 3, 4, 5, 255, 256, 257, 1027, 4099, 262147]
FILL_VOXELS = VOXELS + [1048583]
STREAMS = [0, 1, 3 * 2 ** 24 + 7, 2 ** 40 + 5, 2 ** 63 - 1]
# |z - z64| <= C_BOUND 2^-24 r, r = sqrt(-2 ln u1), from the documented 1-ulp bounds of logf, sqrtf
# and sincospif, the rounding of u2 (an angle error of up to 2 pi 2^-25) and the final product
C_BOUND = 9.2


def np_(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def same(a, b):
    """bit for bit, NaN-aware"""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def bits(key, draw, quads):
    out = torch.empty((key.n, quads, 4), dtype=torch.int32, device="cuda")
    H.check(H.load().ddpm3d_noise_bits(key.desc(draw), key.n, quads, H.ptr(out), H.stream()))
    return np_(out).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. the generator
@pytest.mark.parametrize("seed", [0, 10, 2 ** 64 - 1])
def test_bits_equal_the_reference_exactly(seed):
    key = NoiseKey(seed, STREAMS)
    for draw in (0, 1, 2 ** 32 - 1):
        got = bits(key, draw, 1028)
        for n, stream in enumerate(STREAMS):
            assert np.array_equal(got[n], NR.words(seed, stream, draw, 1028)), (seed, stream, draw)


# ---------------------------------------------------------------------------------------------- 2. the normals
@pytest.fixture(scope="module")
def fills():
    """(N = 3, voxels) fills of draw 1, seed 10, per size: computed once, read by the tests below"""
    key = NoiseKey(10, [0, 3 * 2 ** 24 + 7, 2 ** 63 - 1])
    return key, {v: key.fill(1, (3, v)) for v in FILL_VOXELS}


@pytest.mark.parametrize("voxels", FILL_VOXELS)
def test_fill_within_the_derived_bound_of_the_fp64_reference(fills, voxels):
    """Measured on an MI355X: see DESIGN.md 3.16 for the share of the bound used."""
    key, out = fills
    got = np_(out[voxels]).astype(np.float64)
    assert got.shape == (3, voxels)
    worst = 0.0
    for n, stream in enumerate((0, 3 * 2 ** 24 + 7, 2 ** 63 - 1)):
        z64, r = NR.normals(10, stream, 1, voxels, with_r=True)
        err = np.abs(got[n] - z64)
        unit = 2.0 ** -24 * r
        if (unit > 0).any():
            worst = max(worst, float((err[unit > 0] / unit[unit > 0]).max()))
        assert (err <= C_BOUND * unit).all(), (voxels, n, float((err - C_BOUND * unit).max()))
    print("voxels %d: largest |z - z64| = %.2f x 2^-24 r (%.0f%% of the bound)" % (voxels, worst, 100 * worst / C_BOUND))
    assert np.abs(got).max() <= np.sqrt(66.0 * np.log(2.0)) * (1 + 1e-6)


# ---------------------------------------------------------------------------------------------- 3. invariance
def test_fill_does_not_depend_on_the_batch_the_length_or_the_call(fills):
    key, out = fills
    for v in (5, 257, 1027, 262147):
        for n in range(3):
            assert torch.equal(key.rows(n, n + 1).fill(1, (1, v)), out[v][n:n + 1]), (v, n)
    assert torch.equal(out[1027][:, :5], out[5])
    assert torch.equal(out[1048583][:, :262147], out[262147])
    assert torch.equal(key.fill(1, (3, 4099)), out[4099])
    assert not torch.equal(key.fill(2, (3, 4099)), out[4099])
    assert not torch.equal(NoiseKey(11, [0, 3 * 2 ** 24 + 7, 2 ** 63 - 1]).fill(1, (3, 4099)), out[4099])
    # a stream given as the int64 of the same bits
    a = NoiseKey(10, [2 ** 64 - 3]).fill(0, (1, 257))
    assert torch.equal(a, NoiseKey(10, torch.tensor([-3], dtype=torch.int64, device="cuda")).fill(0, (1, 257)))


# ---------------------------------------------------------------------------------------------- 4. fusion
def _diffusion(learn_sigma=True):
    return su.create_gaussian_diffusion(steps=1000, learn_sigma=learn_sigma, timestep_respacing="10")


def _inputs(N, voxels, learn_sigma, seed):
    shape = (N, 1, voxels)
    x, m1, m2 = (dev(a) for a in synth.synth_noise(shape, 3, seed=seed))
    mo = dev(synth.synth_model_output(shape, learn_sigma, seed + 1))
    return x, m1.clamp(-1, 1), m2.clamp(-1, 1), mo


def _sample_step(d, ddim, mo, x, t, flags, eta, noise=None, key=None, draw=0):
    lib, st = H.load(), d._device_state(x.device)
    N, vox = x.shape[0], x[0].numel()
    sample, x0 = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    src = key.desc(draw) if key is not None else H.ptr(noise)
    name = ("ddpm3d_ddim_step" if ddim else "ddpm3d_p_sample_step") + ("_keyed" if key is not None else "")
    args = [H.ptr(mo), H.ptr(x), src, H.ptr(st["coef"]), H.ptr(t), N, vox, flags] + ([eta] if ddim else [])
    H.check(getattr(lib, name)(*args, H.ptr(sample), H.ptr(x0), H.stream()))
    return sample, x0


def _solver_step(d, mo, x, m1, m2, t, flags, order, sde_table, keyed, noise=None, key=None, draw=0):
    """One solver launch on the SDE or ODE table: the keyed entry on `key` (None = its ODE form) or the un-keyed one
    on `noise` (None = its ODE form)."""
    lib, st = H.load(), d._device_state(x.device)
    scoef = d._solver_state(x.device, order, sde_table)
    sample, x0 = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    src = (key.desc(draw) if key is not None else None) if keyed else H.ptr(noise)
    fn = lib.ddpm3d_dpm_solver_step_keyed if keyed else lib.ddpm3d_dpm_solver_step
    H.check(fn(H.ptr(mo), H.ptr(x), H.ptr(m1), H.ptr(m2), src, H.ptr(st["coef"]), H.ptr(scoef), H.ptr(t), x.shape[0],
               x[0].numel(), d.num_timesteps, flags, order, H.ptr(sample), H.ptr(x0), H.stream()))
    return sample, x0


def _q_sample(d, xs, t, noise=None, key=None, draw=0):
    lib, st = H.load(), d._device_state(xs.device)
    out = torch.full_like(xs, 7.0)
    if key is not None:
        H.check(lib.ddpm3d_q_sample_keyed(H.ptr(xs), key.desc(draw), H.ptr(st["qcoef"]), H.ptr(t), xs.shape[0],
                                          xs[0].numel(), d.num_timesteps, H.ptr(out), H.stream()))
    else:
        H.check(lib.ddpm3d_q_sample(H.ptr(xs), H.ptr(noise), H.ptr(st["qcoef"]), H.ptr(t), xs.shape[0],
                                    xs[0].numel(), d.num_timesteps, H.ptr(out), H.stream()))
    return out


KEY_STREAMS = [dist_util.noise_stream(4, 0), dist_util.noise_stream(4, 1), dist_util.noise_stream(2 ** 24 + 1, 300)]


def _t(values):
    return torch.tensor(values, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("voxels", [5, 1027, 4096])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("learn_sigma", [True, False])
def test_p_sample_step_keyed_equals_unkeyed_on_the_filled_noise(learn_sigma, clip, voxels):
    d = _diffusion(learn_sigma)
    x, _, _, mo = _inputs(3, voxels, learn_sigma, 71)
    key = NoiseKey(10, KEY_STREAMS)
    z = key.fill(4, x.shape)
    t = _t([9, 0, 4])                                    # the mask of t == 0 among them
    a = _sample_step(d, False, mo, x, t, d._flags(clip), 0.0, key=key, draw=4)
    b = _sample_step(d, False, mo, x, t, d._flags(clip), 0.0, noise=z)
    assert same(a[0], b[0]) and same(a[1], b[1])
    assert torch.isfinite(a[0]).all() and not torch.equal(a[0][0], a[1][0])       # the noise term is live at t = 9


@pytest.mark.parametrize("voxels", [5, 1027, 4096])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_step_keyed_equals_unkeyed_on_the_filled_noise(eta, voxels):
    d = _diffusion()
    x, _, _, mo = _inputs(3, voxels, True, 73)
    key = NoiseKey(10, KEY_STREAMS)
    z = key.fill(2, x.shape)
    t = _t([9, 0, 4])
    a = _sample_step(d, True, mo, x, t, d._flags(True), eta, key=key, draw=2)
    b = _sample_step(d, True, mo, x, t, d._flags(True), eta, noise=z)
    assert same(a[0], b[0]) and same(a[1], b[1]) and torch.isfinite(a[0]).all()


@pytest.mark.parametrize("voxels", [5, 1027, 4096])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_dpm_solver_step_keyed_equals_unkeyed_on_the_filled_noise(order, voxels):
    """The kernel takes any order with noise (the host loop offers the SDE form at orders 1 and 2); the table read is
    that of the loop's own form.  One sample's t is out of range: NaN on both sides.  A NULL key is the ODE form."""
    d = _diffusion()
    x, m1, m2, mo = _inputs(3, voxels, True, 75)
    key = NoiseKey(10, KEY_STREAMS)
    z = key.fill(3, x.shape)
    flags = d._flags(True)
    sde = order < 3
    for t in ([9, 0, 4], [3, 10, 0], [-1, 2, 1 << 40]):
        t = _t(t)
        a = _solver_step(d, mo, x, m1, m2, t, flags, order, sde, True, key=key, draw=3)
        b = _solver_step(d, mo, x, m1, m2, t, flags, order, sde, False, noise=z)
        assert same(a[0], b[0]) and same(a[1], b[1]), t
        ode_keyed = _solver_step(d, mo, x, m1, m2, t, flags, order, False, True)
        ode = _solver_step(d, mo, x, m1, m2, t, flags, order, False, False)
        assert same(ode_keyed[0], ode[0]) and same(ode_keyed[1], ode[1]), t
    assert torch.isnan(a[0][0]).all() and torch.isnan(a[0][2]).all() and torch.isfinite(a[0][1]).all()


@pytest.mark.parametrize("voxels", [5, 1027, 4096])
def test_q_sample_keyed_equals_unkeyed_on_the_filled_noise(voxels):
    d = _diffusion()
    xs = dev(synth.synth_x_start((3, 1, voxels), seed=77))
    key = NoiseKey(10, KEY_STREAMS)
    z = key.fill(9, xs.shape)
    for t in ([9, 0, 4], [3, 10, 0]):
        a = _q_sample(d, xs, _t(t), key=key, draw=9)
        assert same(a, _q_sample(d, xs, _t(t), noise=z)), t
    assert torch.isnan(a[1]).all() and torch.isfinite(a[0]).all() and torch.isfinite(a[2]).all()


# ---------------------------------------------------------------------------------------------- 5. geometry
CANVAS, PATCH = (5, 7, 9), (4, 4, 4)
ORIGINS = [(0, 0, 0), (1, 3, 5), (1, 2, 3)]


def _patch_key(origins):
    """the key of the patches at `origins` x 2 draws, patch-major: draw k's canvas is stream noise_stream(0, k)"""
    rows = [(o, k) for o in origins for k in range(2)]
    return NoiseKey(10, [dist_util.noise_stream(0, k) for _, k in rows], origin=[o for o, _ in rows], patch=PATCH,
                    canvas=CANVAS)


def _geometry(origins, draw):
    """K = 2 canvases of `draw` from ddpm3d_noise_fill, the patches' key, and the patches gathered from the canvases"""
    canvases = joint.draw_key(10, 2, "cuda").fill(draw, (2,) + CANVAS)
    gathered = torch.stack([canvases[k, z0:z0 + 4, y0:y0 + 4, x0:x0 + 4] for z0, y0, x0 in origins for k in range(2)])
    return canvases, _patch_key(origins), gathered.reshape(2 * len(origins), 1, 64).contiguous()


def test_canvas_fill_is_the_reference_at_the_canvas_index():
    canvases, pkey, gathered = _geometry(ORIGINS, 3)
    ref = NR.normals(10, dist_util.noise_stream(0, 1), 3, int(np.prod(CANVAS)))
    idx = NR.canvas_index(ORIGINS[1], PATCH, CANVAS)
    got = np_(gathered[3]).reshape(PATCH).astype(np.float64)                  # patch 1, draw 1
    assert np.abs(got - ref[idx]).max() <= C_BOUND * 2.0 ** -24 * 6.77
    assert torch.equal(pkey.fill(3, gathered.shape), gathered)                # the fill's per-voxel form


@pytest.mark.parametrize("entry", ["p_sample_step", "ddim_step", "dpm_solver_step", "q_sample"])
def test_keyed_step_with_origins_equals_the_step_on_gathered_canvas_noise(entry):
    """Then one origin, (2, 0, 0), puts its patch outside the 5-deep canvas: those samples are all NaN, the others
    keep their bits."""
    d = _diffusion()
    N = 2 * len(ORIGINS)
    x, m1, m2, mo = _inputs(N, 64, True, 79)
    t = _t([9, 4, 0, 7, 2, 9])
    flags = d._flags(True)

    def run(key=None, noise=None):
        kw = dict(key=key, draw=3) if key is not None else dict(noise=noise)
        if entry == "p_sample_step":
            return _sample_step(d, False, mo, x, t, flags, 0.0, **kw)
        if entry == "ddim_step":
            return _sample_step(d, True, mo, x, t, flags, 0.5, **kw)
        if entry == "dpm_solver_step":
            return _solver_step(d, mo, x, m1, m2, t, flags, 2, True, key is not None, **kw)
        return (_q_sample(d, x, t, **kw),)

    _, pkey, gathered = _geometry(ORIGINS, 3)
    good = run(key=pkey)
    for a, b in zip(good, run(noise=gathered)):
        assert same(a, b) and torch.isfinite(a).all()
    for a, g in zip(run(key=_patch_key([ORIGINS[0], (2, 0, 0), ORIGINS[2]])), good):
        assert torch.isnan(a[2:4]).all()
        assert torch.equal(a[:2], g[:2]) and torch.equal(a[4:], g[4:])
    for origin in ((-1, 0, 0), (0, 4, 0), (0, 0, 6), (2 ** 31 - 1, 0, 0)):
        assert torch.isnan(_patch_key([origin]).fill(3, (2, 1, 64))).all(), origin


# ---------------------------------------------------------------------------------------------- 6. loops
@pytest.fixture(scope="module")
def tiny():
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(TINY)
    fl["timestep_respacing"] = "3"
    model, diff = su.sr_create_model_and_diffusion(**fl)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape)))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    shape = (2, 1, 16, 16, 16)
    low = dev(synth.synth_low_res(shape, seed=1234))
    key = NoiseKey(10, [dist_util.noise_stream(5, 0), dist_util.noise_stream(6, 2)])
    return model, diff, shape, low, key


@pytest.mark.parametrize("loop, extra", [("p_sample_loop", {}), ("ddim_sample_loop", dict(eta=0.5)),
                                         ("dpm_solver_sample_loop", dict(order=2, stochastic=True))])
def test_sampling_loop_with_a_key_equals_the_loop_on_the_filled_tensors(tiny, loop, extra):
    model, diff, shape, low, key = tiny
    fn = getattr(diff, loop)
    keyed = fn(model, shape, model_kwargs={"low_res": low}, noise_key=key, **extra)
    explicit = fn(model, shape, noise=key.fill(0, shape), model_kwargs={"low_res": low},
                  step_noise=[key.fill(k + 1, shape) for k in range(3)], **extra)
    assert torch.equal(keyed, explicit) and torch.isfinite(keyed).all() and float(keyed.abs().max()) > 0
    # every step, both outputs
    steps = list(getattr(diff, loop + "_progressive")(model, shape, model_kwargs={"low_res": low}, noise_key=key,
                                                      **extra))
    assert len(steps) == 3 and torch.equal(steps[-1]["sample"], keyed)
    with pytest.raises(ValueError, match="noise_key"):
        fn(model, shape, model_kwargs={"low_res": low}, noise_key=key, step_noise=[None] * 3, **extra)


def test_solver_ode_loop_takes_x_T_from_the_key(tiny):
    model, diff, shape, low, key = tiny
    a = diff.dpm_solver_sample_loop(model, shape, model_kwargs={"low_res": low}, noise_key=key)
    b = diff.dpm_solver_sample_loop(model, shape, noise=key.fill(0, shape), model_kwargs={"low_res": low})
    assert torch.equal(a, b)


def test_calc_bpd_loop_with_a_key_equals_the_loop_on_the_filled_tensors(tiny):
    model, diff, shape, low, key = tiny
    xs = dev(synth.synth_x_start(shape, seed=21))
    keyed = diff.calc_bpd_loop(model, xs, model_kwargs={"low_res": low}, noise_key=key)
    explicit = diff.calc_bpd_loop(model, xs, model_kwargs={"low_res": low},
                                  step_noise=[key.fill(k + 1, shape) for k in range(3)])
    for name in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        assert torch.equal(keyed[name], explicit[name]) and torch.isfinite(keyed[name]).all(), name
    # the single-step forms
    t = _t([2, 0])
    assert torch.equal(diff.q_sample(xs, t, noise_key=key, draw=7), diff.q_sample(xs, t, noise=key.fill(7, shape)))
    a = diff.p_sample(model, xs, t, model_kwargs={"low_res": low}, noise_key=key, draw=7)
    b = diff.p_sample(model, xs, t, model_kwargs={"low_res": low}, noise=key.fill(7, shape))
    assert torch.equal(a["sample"], b["sample"]) and torch.equal(a["pred_xstart"], b["pred_xstart"])
    a = diff.ddim_sample(model, xs, t, model_kwargs={"low_res": low}, eta=1.0, noise_key=key, draw=7)
    b = diff.ddim_sample(model, xs, t, model_kwargs={"low_res": low}, eta=1.0, noise=key.fill(7, shape))
    assert torch.equal(a["sample"], b["sample"])


@pytest.mark.parametrize("kind, eta, overlap", [("ddpm", 0.0, None), ("ddim", 0.5, None), ("ddpm", 0.0, 6)])
def test_joint_loop_with_a_key_equals_the_loop_on_explicit_canvases(tiny, kind, eta, overlap):
    """The geometry of tests/test_gpu_joint.py, K = 2 draws, and the same volume on the sliding grid.  The keyed loop
    draws, holds and gathers no noise canvas; its patches read the canvas voxel's normal in the step kernel."""
    model, diff, _, _, _ = tiny
    geom = patches.joint_geometry((20, 40, 40), 16, min_overlap=overlap)
    low = synth.synth_low_res((20, 40, 40), seed=1234)
    key = joint.draw_key(10, 2, "cuda")
    cshape = (2,) + tuple(geom.canvas)
    common = dict(kind=kind, num_draws=2, batch_size=4, eta=eta, device="cuda")
    keyed = joint.sample_loop(diff, model, low, geom, noise_key=key, **common)
    explicit = joint.sample_loop(diff, model, low, geom, noise=key.fill(0, cshape),
                                 step_noise=[key.fill(k + 1, cshape) for k in range(3)], **common)
    assert keyed.shape == cshape and torch.equal(keyed, explicit) and torch.isfinite(keyed).all()
    assert not torch.equal(keyed[0], keyed[1])
    # neither the batch size nor the draw count moves a draw
    one = joint.sample_loop(diff, model, low, geom, noise_key=joint.draw_key(10, 1, "cuda"), kind=kind, num_draws=1,
                            batch_size=3, eta=eta, device="cuda")
    assert float((one[0] - keyed[0]).abs().max()) <= 1e-3 * float(keyed[0].abs().max())
    with pytest.raises(ValueError):
        joint.sample_loop(diff, model, low, geom, noise_key=joint.draw_key(10, 3, "cuda"), **common)
