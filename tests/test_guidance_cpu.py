"""
CPU tier of the low-pass data-consistency guidance: the fp32 yardstick of the operator and of the
guided steps (tests/guidance_ref.py) is pinned to the reference's own p_sample and ddim_sample run with that operator as
denoised_fn (tests/golden/guidance.npz, make_golden_guidance.py); the C ABI declares and exports the new entries and
refuses bad arguments on the host before any HIP call; the Python layer refuses a bad guide before the model is called;
the pull's taps are metrics.gaussian_taps'.  No GPU is touched here.
"""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref as gr
from conftest import PKG, ROOT
from guided_diffusion import _hip
from guided_diffusion import guidance, joint, metrics, patches, synth
from guided_diffusion import script_util as su

NEW = ["ddpm3d_xstart_pull_workspace_bytes", "ddpm3d_xstart_pull", "ddpm3d_p_sample_step_x0", "ddpm3d_ddim_step_x0",
       "ddpm3d_dpm_solver_step_x0"]
FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
SEEDS = dict(x=22, model_output=23, measurement=77, noise=78)        # make_golden_guidance.SEEDS
K_SHAPE = (3, 1, 4, 16, 16)
K_VARIANTS = {"learned_range": dict(learn_sigma=True), "fixed_large": dict(learn_sigma=False),
              "fixed_small": dict(learn_sigma=False, sigma_small=True),
              "xstart": dict(learn_sigma=True, predict_xstart=True)}
RADII = {"r123": (1, 2, 3), "r000": (0, 0, 0)}


def golden_inputs(variant):
    over = K_VARIANTS[variant]
    x = torch.from_numpy(synth.synth_noise(K_SHAPE, 1, seed=SEEDS["x"])[0])
    y = torch.from_numpy(synth.synth_low_res(K_SHAPE, seed=SEEDS["measurement"]))
    z = torch.from_numpy(synth.synth_noise(K_SHAPE, 1, seed=SEEDS["noise"])[0])
    mo = torch.from_numpy(synth.synth_model_output(K_SHAPE, over["learn_sigma"], SEEDS["model_output"]))
    return x, y, z, mo


# ---------------------------------------------------------------------------------- the yardstick against the reference
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("rtag", sorted(RADII))
@pytest.mark.parametrize("variant", sorted(K_VARIANTS))
def test_yardstick_is_the_references_denoised_fn_path(golden, variant, rtag, clip):
    """guidance_ref's pulled x0 and its DDIM steps (eta 0 and 0.5) equal the reference's bit for bit; its DDPM step,
    where the host's exp enters (exp(0.5 logvar) noise), within an ulp of exp: two ulps of that term (the exp and the
    product's rounding) plus one of the sample.  On the host that wrote the file the DDPM step is bitwise too."""
    g = golden("guidance.npz")
    key = "%s/%s/%s" % (variant, rtag, "clip" if clip else "noclip")
    over = K_VARIANTS[variant]
    d = su.create_gaussian_diffusion(steps=1000, timestep_respacing="250", **over)
    coef = d.coef_table()
    x, y, z, mo = golden_inputs(variant)
    t = torch.from_numpy(g["t"])
    w = float(g["weight"])
    x0 = gr.pulled_x0(coef, mo, x, t, y, gr.taps_for(RADII[rtag]), w, over.get("predict_xstart", False), clip)
    assert np.array_equal(x0.numpy(), g[key + "/pred_xstart"])
    for eta in (0.0, 0.5):
        assert np.array_equal(gr.ddim_step(coef, x, t, z, x0, eta).numpy(), g[key + "/ddim_eta%g" % eta]), eta
    got = gr.p_sample_step(coef, mo, x, t, z, x0, over["learn_sigma"]).numpy()
    ref = g[key + "/p_sample"]
    mean = (torch.from_numpy(coef[:, 2])[t].reshape(-1, 1, 1, 1, 1) * x0
            + torch.from_numpy(coef[:, 3])[t].reshape(-1, 1, 1, 1, 1) * x).numpy()
    allowed = 2 * np.spacing(np.abs(ref - mean)) + np.spacing(np.abs(ref))
    assert (np.abs(got - ref) <= allowed).all()


def test_fma32_rounds_once():
    """the fused sum against exact rational arithmetic, on operands chosen to sit near fp32 midpoints"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    t = np.float32(0.3)
    x = rng.standard_normal(4096).astype(np.float32)
    acc = (-(np.float64(t) * x) + rng.integers(-3, 4, 4096) * 2.0 ** -25 * np.abs(x)).astype(np.float32)
    got = gr.fma32(t, x, acc)
    for i in range(0, 4096, 7):
        exact = Fraction(float(t)) * Fraction(float(x[i])) + Fraction(float(acc[i]))
        lo = np.float32(float(exact))
        cands = sorted({float(lo), float(np.nextafter(lo, np.float32(np.inf))),
                        float(np.nextafter(lo, np.float32(-np.inf)))}, key=lambda c: abs(Fraction(c) - exact))
        assert abs(Fraction(float(got[i])) - exact) == abs(Fraction(cands[0]) - exact), i


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _hip.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13


def _taps(values):
    return (ctypes.c_float * len(values))(*values)


def _pull_args(**over):
    a = dict(model_out=FAKE, x=2 * FAKE, measurement=3 * FAKE, coef=4 * FAKE, t_idx=5 * FAKE, N=2, D=4, H=8, W=8, T=10,
             flags=_hip.F_LEARN_SIGMA | _hip.F_CLIP, weight=0.5, r0=1, r1=0, r2=2, taps0=_taps([0.5, 1.0, 0.5]),
             taps1=_taps([1.0]), taps2=_taps([0.1, 0.5, 1.0, 0.5, 0.1]), xstart_out=6 * FAKE, ws=7 * FAKE,
             ws_bytes=2 * 4 * 8 * 8 * 4, stream=None)
    a.update(over)
    return list(a.values())


def test_pull_workspace_bytes():
    lib = _hip.load()
    assert lib.ddpm3d_xstart_pull_workspace_bytes(2, 4, 8, 8) == 2 * 4 * 8 * 8 * 4
    assert lib.ddpm3d_xstart_pull_workspace_bytes(1, 1, 1, 1) == 16
    for bad in ((0, 4, 8, 8), (2, 0, 8, 8), (2, 4, -1, 8), (2, 4, 8, 0), (65536, 1, 1, 1), (2, 1024, 1024, 1024),
                (1, 1 << 16, 1 << 16, 1)):
        assert lib.ddpm3d_xstart_pull_workspace_bytes(*bad) == 0, bad


@pytest.mark.parametrize("over", [
    dict(model_out=None), dict(x=None), dict(measurement=None), dict(coef=None), dict(t_idx=None), dict(taps0=None),
    dict(taps1=None), dict(taps2=None), dict(xstart_out=None), dict(ws=None),
    dict(N=0), dict(N=65536), dict(D=0), dict(H=-1), dict(W=0), dict(T=0), dict(N=4, D=1024, H=1024, W=1024),
    dict(flags=8), dict(r0=-1), dict(r2=17),
    dict(taps0=_taps([0.5, 1.0, 0.25])), dict(taps0=_taps([0.0, 1.0, 0.0])), dict(taps0=_taps([-0.5, 1.0, -0.5])),
    dict(taps2=_taps([0.1, 0.5, float("inf"), 0.5, 0.1])), dict(taps1=_taps([float("nan")])),
    dict(weight=-0.01), dict(weight=1.5), dict(weight=float("nan")), dict(weight=float("inf")),
    dict(ws_bytes=2 * 4 * 8 * 8 * 4 - 16), dict(ws=7 * FAKE + 4),
    dict(xstart_out=FAKE), dict(xstart_out=2 * FAKE), dict(xstart_out=3 * FAKE), dict(xstart_out=FAKE + 2048 + 64),
    dict(ws=6 * FAKE), dict(ws=FAKE), dict(ws=3 * FAKE),
])
def test_xstart_pull_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_xstart_pull(*_pull_args(**over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("xstart_pull:")


def _step_args(kind, **over):
    key = _hip.NoiseKeyDesc()
    key.seed, key.stream, key.draw = 1, FAKE, 1
    a = dict(model_out=FAKE, xstart=2 * FAKE, x=3 * FAKE)
    if kind == "dpm_solver":
        a.update(x0_prev1=8 * FAKE, x0_prev2=9 * FAKE)
    a.update(noise=4 * FAKE, key=None, coef=5 * FAKE)
    if kind == "dpm_solver":
        a.update(scoef=10 * FAKE)
    a.update(t_idx=6 * FAKE, N=2, voxels=64)
    if kind == "dpm_solver":
        a.update(T=10)
    a.update(flags=_hip.F_LEARN_SIGMA)
    if kind == "ddim":
        a.update(eta=0.5)
    if kind == "dpm_solver":
        a.update(order=3)
    a.update(sample=7 * FAKE, pred_xstart=11 * FAKE, stream=None)
    if over.pop("keyed", False):
        a.update(noise=None, key=key)
    a.update(over)
    return list(a.values())


COMMON_BAD = [dict(xstart=None), dict(x=None), dict(coef=None), dict(t_idx=None), dict(sample=None), dict(N=0),
              dict(N=65536), dict(voxels=0), dict(flags=8), dict(keyed=True, noise=4 * FAKE),
              dict(sample=11 * FAKE), dict(sample=2 * FAKE), dict(sample=3 * FAKE), dict(pred_xstart=2 * FAKE),
              dict(pred_xstart=3 * FAKE), dict(sample=4 * FAKE), dict(keyed=True, N=0)]


@pytest.mark.parametrize("over", COMMON_BAD + [dict(noise=None), dict(model_out=None)])
def test_p_sample_step_x0_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_p_sample_step_x0(*_step_args("ddpm", **over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("p_sample_step_x0:")


@pytest.mark.parametrize("over", COMMON_BAD + [dict(noise=None)])
def test_ddim_step_x0_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_ddim_step_x0(*_step_args("ddim", **over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("ddim_step_x0:")


@pytest.mark.parametrize("over", COMMON_BAD + [dict(scoef=None), dict(pred_xstart=None), dict(T=0), dict(order=0),
                                               dict(order=4), dict(x0_prev1=None), dict(x0_prev2=None),
                                               dict(sample=8 * FAKE), dict(pred_xstart=9 * FAKE)])
def test_dpm_solver_step_x0_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_dpm_solver_step_x0(*_step_args("dpm_solver", **over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("dpm_solver_step_x0:")


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_pull_taps_are_gaussian_taps():
    for fwhm, spacing in ((8.0, (2.0, 2.0, 2.0)), (6.0, (3.27, 2.0, 1.5)), (1.0, (4.0, 4.0, 4.0))):
        pull = guidance.LowPassPull(fwhm, spacing)
        ref = metrics.gaussian_taps(fwhm, spacing)
        assert pull.radii == ref.radii and pull.taps.taps == ref.taps and pull.taps.sigma_voxels == ref.sigma_voxels
    assert guidance.LowPassPull(8.0, (2.0, 2.0, 2.0)).radii == (5, 5, 5)
    zero = guidance.LowPassPull(0, None)
    assert zero.radii == (0, 0, 0) and zero.taps.taps == ((1.0,),) * 3
    assert guidance.LowPassPull(0.0, (2.0, 2.0, 2.0), weight=0.37).weight == float(np.float32(0.37))


@pytest.mark.parametrize("args, kw, match", [
    ((-1.0, (2, 2, 2)), {}, "fwhm_mm"), ((float("nan"), (2, 2, 2)), {}, "fwhm_mm"),
    ((float("inf"), (2, 2, 2)), {}, "fwhm_mm"), (("8", (2, 2, 2)), {}, "fwhm_mm"),
    ((8.0, None), {}, "spacing"), ((8.0, (2, 2)), {}, "spacing"), ((8.0, (2, 0, 2)), {}, "spacing"),
    ((80.0, (2, 2, 1)), {}, "radius"),
    ((8.0, (2, 2, 2)), dict(weight=-0.1), "weight"), ((8.0, (2, 2, 2)), dict(weight=1.01), "weight"),
    ((8.0, (2, 2, 2)), dict(weight=float("nan")), "weight"), ((8.0, (2, 2, 2)), dict(weight=None), "weight"),
    ((8.0, (2, 2, 2)), dict(stop_t=-1), "stop_t"), ((8.0, (2, 2, 2)), dict(stop_t=1.5), "stop_t"),
    ((8.0, (2, 2, 2)), dict(stop_t=True), "stop_t"), ((8.0, (2, 2, 2)), dict(measurement=[1.0]), "measurement"),
])
def test_pull_refuses_bad_parameters(args, kw, match):
    with pytest.raises(ValueError, match=match):
        guidance.LowPassPull(*args, **kw)


class _Model:
    """Records calls; any call is a failure of the tests below."""

    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("the model must not be called")

    def parameters(self):
        return iter([torch.zeros(1)])


def _every_entry(d, m, shape, guide, model_kwargs):
    """one call per public entry that takes guide="""
    x, t = torch.zeros(shape), torch.tensor([3] * shape[0])
    yield lambda: d.p_sample(m, x, t, model_kwargs=model_kwargs, guide=guide)
    yield lambda: d.ddim_sample(m, x, t, model_kwargs=model_kwargs, guide=guide)
    yield lambda: d.p_sample_loop(m, shape, model_kwargs=model_kwargs, guide=guide)
    yield lambda: next(d.p_sample_loop_progressive(m, shape, model_kwargs=model_kwargs, guide=guide))
    yield lambda: d.ddim_sample_loop(m, shape, model_kwargs=model_kwargs, guide=guide)
    yield lambda: next(d.ddim_sample_loop_progressive(m, shape, model_kwargs=model_kwargs, guide=guide))
    yield lambda: d.dpm_solver_sample_loop(m, shape, model_kwargs=model_kwargs, guide=guide)
    yield lambda: next(d.dpm_solver_sample_loop_progressive(m, shape, model_kwargs=model_kwargs, guide=guide))


def test_a_bad_guide_is_refused_before_the_model_runs():
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="ddim10")
    m = _Model()
    shape = (1, 1, 4, 8, 8)
    pull = guidance.LowPassPull(8.0, (2.0, 2.0, 2.0))
    low = torch.zeros(shape)
    cases = [
        (lambda v: v, {"low_res": low}, "LowPassPull"),                                  # not a pull
        (pull, {}, "low_res"),                                                           # no measurement at all
        (pull, None, "low_res"),
        (pull, {"low_res": torch.zeros((1, 1, 4, 8, 9))}, "shape"),                      # not x's shape
        (guidance.LowPassPull(8.0, (2.0, 2.0, 2.0), measurement=torch.zeros((2, 1, 4, 8, 8))), {"low_res": low},
         "shape"),
    ]
    for guide, kw, match in cases:
        for call in _every_entry(d, m, shape, guide, kw):
            with pytest.raises(ValueError, match=match):
                call()
    for call in _every_entry(d, m, (1, 3, 8, 8), pull, {"low_res": torch.zeros((1, 3, 8, 8))}):
        with pytest.raises(ValueError, match=r"\(N, 1, D, H, W\)"):
            call()
    assert m.calls == 0


def test_hooks_stay_refused_with_a_guide():
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="ddim10")
    m = _Model()
    shape = (1, 1, 4, 8, 8)
    pull = guidance.LowPassPull(0, None)
    kw = {"low_res": torch.zeros(shape)}
    fn = lambda v: v  # noqa: E731
    with pytest.raises(NotImplementedError):
        d.p_sample_loop(m, shape, model_kwargs=kw, denoised_fn=fn, guide=pull)
    with pytest.raises(NotImplementedError):
        d.ddim_sample_loop(m, shape, model_kwargs=kw, cond_fn=fn, guide=pull)
    with pytest.raises(NotImplementedError):
        d.dpm_solver_sample_loop(m, shape, model_kwargs=kw, denoised_fn=fn, guide=pull)
    assert m.calls == 0


def test_joint_loop_refuses_a_measurement_and_a_non_pull():
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="ddim10")
    m = _Model()
    g = patches.joint_geometry((20, 40, 40), 16)
    vol = np.zeros((20, 40, 40), dtype=np.float32)
    with pytest.raises(ValueError, match="measurement"):
        joint.sample_loop(d, m, vol, g, guide=guidance.LowPassPull(0, None, measurement=torch.zeros((1, 1, 16, 16, 16))))
    with pytest.raises(ValueError, match="LowPassPull"):
        joint.sample_loop(d, m, vol, g, guide=lambda v: v)
    assert m.calls == 0


def test_active_steps_follow_the_original_timestep():
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="ddim10")
    tmap = list(d.timestep_map)
    pull = guidance.LowPassPull(0, None, stop_t=tmap[4])
    assert [pull.active(d, i) for i in range(10)] == [False] * 4 + [True] * 6
    assert all(guidance.LowPassPull(0, None).active(d, i) for i in range(10))
    assert not any(guidance.LowPassPull(0, None, weight=0.0).active(d, i) for i in range(10))
    plain = su.create_gaussian_diffusion(steps=100, learn_sigma=True, timestep_respacing="")
    assert [guidance.LowPassPull(0, None, stop_t=98).active(plain, i) for i in (97, 98, 99)] == [False, True, True]


# ------------------------------------------------------------------------------------------------------------ the script
def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SPACED = ["--voxel_spacing", "2", "2", "2"]


@pytest.mark.parametrize("flags, message", [
    (["--consistency_fwhm", "-1"] + SPACED, "--consistency_fwhm must be a finite number of mm"),
    (["--consistency_fwhm", "nan"] + SPACED, "--consistency_fwhm must be a finite number of mm"),
    (["--consistency_fwhm", "inf"] + SPACED, "--consistency_fwhm must be a finite number of mm"),
    (["--consistency_fwhm", "8", "--consistency_weight", "1.5"] + SPACED, "--consistency_weight must be in [0, 1]"),
    (["--consistency_fwhm", "8", "--consistency_weight", "-0.1"] + SPACED, "--consistency_weight must be in [0, 1]"),
    (["--consistency_fwhm", "8", "--consistency_weight", "nan"] + SPACED, "--consistency_weight must be in [0, 1]"),
    (["--consistency_fwhm", "8", "--consistency_stop_t", "-1"] + SPACED, "--consistency_stop_t must not be negative"),
    (["--consistency_fwhm", "80"] + SPACED, "DDPM3D_SMOOTH_MAX_RADIUS"),
    (["--consistency_fwhm", "8"], "--consistency_fwhm needs --voxel_spacing"),
    (["--consistency_weight", "0.5"], "need --consistency_fwhm"),
    (["--consistency_stop_t", "100"], "need --consistency_fwhm"),
])
def test_script_refuses_bad_consistency_flags_before_the_model_is_built(tmp_path, capsys, monkeypatch, flags, message):
    mod = _script()
    monkeypatch.setattr(mod, "sr_create_model_and_diffusion",
                        lambda **kw: (_ for _ in ()).throw(AssertionError("the model must not be built")))
    src = tmp_path / "pet.npy"
    np.save(src, np.zeros((16, 16, 16), dtype=np.float32))
    with pytest.raises(SystemExit) as e:
        mod.main(["--base_samples", str(src), "--save_dir", str(tmp_path / "o")] + flags)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
