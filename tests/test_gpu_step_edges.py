"""
The DDPM / DDIM step kernel (sample_step_kernel behind ddpm3d_p_sample_step, ddpm3d_ddim_step and their _keyed and
_x0 forms) at its edges, element by element against tests/step_ref.py, the op-by-op fp32 restatement of the
reference's p_sample and ddim_sample: every flag combination, one t per sample with the masked step among unmasked
ones, the respaced and the unspaced schedule, one voxel to a second grid pass with a ragged tail, the _x0 entries with
NaN in what they must not read, NaN and +-Inf through the step, NULL pred_xstart -- and NaN through the clip of every
other kernel that derives x0 the same way.  Cases, inputs and comparator are step_ref's, where
tests/test_step_ref_cpu.py shows that the comparator sees nine kinds of kernel error on these inputs.

Bars (step_ref.check, u = 2^-24), per element, nothing excluded, NaN pattern equal to the reference's:
  pred_xstart, every DDIM sample, the DDPM sample of a row at t == 0: bit-equal.  Add, multiply, divide and sqrtf are
  IEEE operations here: the library is built without fast-math flags, contraction is off in the step section, and
  hipcc's default for HIP, correctly rounded fp32 divide and square root, is in force (the device compile of ops.hip
  carries no -fno-hip-fp32-correctly-rounded-divide-sqrt and links OCML's correctly_rounded_sqrt_on, unsafe_math_off,
  finite_only_off and daz_opt_off control libraries).
  DDPM sample of a row at t > 0: |got - ref| <= 4u |sigma z| + 2u |ref|.  expf is the one operation that is not
  correctly rounded: 1 ulp, the figure the formula is written for, is what HIP's published math API table gives
  for expf (the table DESIGN.md 3.16 takes logf, sqrtf and sincospif from).  tests/test_gpu_ddim_reverse.py holds
  the same expf to 1 ulp of the reference's exp, voxel by voxel.

No launch here gives the kernel a t outside [0, T): it takes no T and would read past the coefficient table.  What
p_sample / ddim_sample do with such a t is tested on the host (tests/test_step_ref_cpu.py).
"""

import numpy as np
import pytest
import torch

import step_ref as SR
from guided_diffusion import _hip as H
from guided_diffusion import script_util as su
from guided_diffusion.gaussian_diffusion import NoiseKey

pytestmark = pytest.mark.gpu

F = np.float32
U = SR.U


def np_(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).cuda()


def nans(like):
    return torch.full_like(like, float("nan"))


def diffusion(respacing, learn_sigma, predict_xstart=False, sigma_small=False):
    return su.create_gaussian_diffusion(steps=1000, learn_sigma=learn_sigma, predict_xstart=predict_xstart,
                                        sigma_small=sigma_small, timestep_respacing=respacing)


# ------------------------------------------------------------------------------------- the step against step_ref
@pytest.mark.parametrize("name", [c["name"] for c in SR.CASES])
def test_step_equals_the_restatement_element_by_element(name):
    case = next(c for c in SR.CASES if c["name"] == name)
    d = diffusion(case["respacing"], case["learn"], case["px"], case["sigma_small"])
    T = d.num_timesteps
    for label, kw in SR.launches(case):
        assert all(0 <= v < T for v in kw["t"])
        if kw["x"].size >= 255:              # three values cannot hold a share of a third
            share = SR.share_of(kw)
            assert 0.10 <= share <= 0.60, (label, share)
        ref = SR.step(**kw)
        x = dev(kw["x"][:, None])
        out = (nans(x), nans(x))             # an element the kernel leaves unwritten stays NaN
        got = d._update(kw["kind"], dev(kw["mo"]), x, torch.tensor(kw["t"]), dev(kw["z"][:, None]), kw["clip"],
                        kw["eta"], out=out, xstart=None if kw["xstart"] is None else dev(kw["xstart"][:, None]))
        assert got["sample"] is out[0] and got["pred_xstart"] is out[1]
        fails = SR.check(kw["kind"], np_(out[0])[:, 0], np_(out[1])[:, 0], ref, kw["t"])
        assert fails == {}, (label, fails)


# ------------------------------------------------------------------------------------------ pred_xstart == NULL
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("ddim", [False, True])
def test_null_pred_xstart_leaves_the_sample_unchanged(ddim, keyed):
    """include/ddpm3d.h lets the plain and the keyed entries run without a pred_xstart buffer."""
    d = diffusion("10", True)
    t = [9, 0, 4]
    mo, x, z = (dev(a) for a in SR.inputs("10", 3, 257, t, True, False, 31))
    key = NoiseKey(10, [3, 5, 2 ** 40 + 1])
    lib, st = H.load(), d._device_state(x.device)
    tt = torch.tensor(t, dtype=torch.int64, device="cuda")
    name = ("ddpm3d_ddim_step" if ddim else "ddpm3d_p_sample_step") + ("_keyed" if keyed else "")

    def run(x0):
        sample = nans(x)
        args = [H.ptr(mo), H.ptr(x), key.desc(2) if keyed else H.ptr(z), H.ptr(st["coef"]), H.ptr(tt), 3, 257,
                d._flags(True)] + ([0.7] if ddim else [])
        H.check(getattr(lib, name)(*args, H.ptr(sample), None if x0 is None else H.ptr(x0), H.stream()))
        return sample

    x0 = nans(x)
    with_buffer = run(x0)
    without = run(None)
    assert torch.isfinite(with_buffer).all() and torch.isfinite(x0).all()
    assert torch.equal(with_buffer, without)


# ------------------------------------------------------------------- NaN through the clip of the other x0 users
def _poisoned(seed, t, respacing, voxels=257):
    """learned-sigma inputs at t with NaN, +Inf and -Inf scattered into both halves of the model output"""
    mo, x, z = SR.inputs(respacing, len(t), voxels, t, True, False, seed)
    return SR.scatter(mo, seed + 1), x, z


# 257 voxels, and a second pass of the grid-stride loop these kernels share with the step kernel (step_grid)
SIZES = [257, SR.STRIDE + 257]


@pytest.mark.parametrize("voxels", SIZES)
@pytest.mark.parametrize("clip", [True, False])
def test_p_mean_variance_keeps_nan_through_the_clip(clip, voxels):
    """mean, log_variance and pred_xstart are the restatement's bit for bit, NaN for NaN; the variance is expf of the
    log-variance, 1 ulp <= 2u of the correctly rounded value."""
    t = [9, 0, 4]
    d = diffusion("10", True)
    mo, x, z = _poisoned(41, t, "10", voxels)
    ref = SR.step("ddpm", "10", mo, x, z, t, True, False, clip)
    got = d._p_mean_variance(dev(mo), dev(x[:, None]), torch.tensor(t, device="cuda"), d._flags(clip))
    for name in ("mean", "log_variance", "pred_xstart"):
        assert SR.compare(np_(got[name])[:, 0], ref[name]) == 0, name
    with np.errstate(all="ignore"):
        var = np.exp(ref["log_variance"].astype(np.float64)).astype(F)
    assert SR.compare(np_(got["variance"])[:, 0], var, 2 * U * np.abs(var.astype(np.float64))) == 0
    assert np.isnan(ref["pred_xstart"]).sum() == 9 and np.isnan(ref["mean"]).any()


@pytest.mark.parametrize("voxels", SIZES)
@pytest.mark.parametrize("clip", [True, False])
def test_ddim_reverse_step_keeps_nan_through_the_clip(clip, voxels):
    t = [9, 0, 4]
    d = diffusion("10", True)
    mo, x, _ = _poisoned(43, t, "10", voxels)
    ref = SR.reverse_step("10", mo, x, t, clip)
    got = d._reverse_step(dev(mo), dev(x[:, None]), torch.tensor(t, device="cuda"), d._flags(clip))
    for name in ("sample", "pred_xstart"):
        assert SR.compare(np_(got[name])[:, 0], ref[name]) == 0, name
    assert np.isnan(ref["sample"]).sum() >= 9


@pytest.mark.parametrize("clip", [True, False])
def test_dpm_solver_step_keeps_nan_through_the_clip(clip):
    """order 1, ODE form: c_x x + w0 x0 on the package's fp32 solver table, two products and one sum"""
    t = [9, 1, 4]
    d = diffusion("10", True)
    mo, x, _ = _poisoned(45, t, "10")
    x0 = SR.step("ddim", "10", mo, x, x, t, True, False, clip)["pred_xstart"]
    tab = d.dpm_solver_table(1, False)[t]
    with np.errstate(all="ignore"):
        sample = tab[:, H.S_CX][:, None] * x + tab[:, H.S_W0][:, None] * x0
    got = d._solver_step(dev(mo), dev(x[:, None]), None, None, None, torch.tensor(t, device="cuda"), d._flags(clip),
                         1, False, 1)
    assert SR.compare(np_(got["pred_xstart"])[:, 0], x0) == 0
    assert SR.compare(np_(got["sample"])[:, 0], sample.astype(F)) == 0
    assert np.isnan(sample).sum() >= 9


@pytest.mark.parametrize("voxels", SIZES)
def test_q_sample_equals_its_two_products_and_one_sum(voxels):
    """sqrt_acp[t] x_0 + sqrt_1m_acp[t] noise (:202-206) from the fp64 tables cast per use, bit for bit, second grid
    pass included; a NaN or an Inf in x_0 goes through as IEEE arithmetic takes it."""
    t = [9, 0, 4]
    d = diffusion("10", True)
    tb = SR.schedule("10")
    rng = np.random.default_rng(49)
    xs = SR.scatter(rng.standard_normal((3, voxels)).astype(F), 50)
    z = rng.standard_normal((3, voxels)).astype(F)
    a, b = (tb[k][t].astype(F)[:, None] for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"))
    with np.errstate(all="ignore"):
        ref = a * xs + b * z
    got = d.q_sample(dev(xs[:, None]), torch.tensor(t), noise=dev(z[:, None]))
    assert SR.compare(np_(got)[:, 0], ref) == 0


@pytest.mark.parametrize("n_bad", [0, 1])
def test_vb_terms_keeps_nan_through_the_clip(n_bad):
    """One NaN in the eps half of one sample -- the decoder-likelihood sample at t == 0 or a KL sample -- makes that
    sample's vb, xstart_mse and mse NaN and leaves the other samples' bits alone."""
    t = [0, 9, 4]
    d = diffusion("10", True)
    mo, x, z = SR.inputs("10", 3, 257, t, True, False, 47)
    xs = np.random.default_rng(48).uniform(-1, 1, x.shape).astype(F)
    tt = torch.tensor(t, dtype=torch.int64, device="cuda")

    def terms(mo):
        vb, xm, mse = (torch.full((3,), 7.0, device="cuda") for _ in range(3))
        xd = dev(x[:, None])
        d._vb_terms(dev(mo), dev(xs[:, None]), xd, tt, dev(z[:, None]), d._flags(True), d._workspace(xd), vb, xm, mse,
                    1, None)
        return [np_(v) for v in (vb, xm, mse)]

    clean = terms(mo)
    bad = mo.copy()
    bad[n_bad, 0, 100] = np.nan
    got = terms(bad)
    others = [n for n in range(3) if n != n_bad]
    for name, a, b in zip(("vb", "xstart_mse", "mse"), got, clean):
        assert np.isfinite(b).all(), name
        assert np.isnan(a[n_bad]), (name, a)
        assert np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32)), name
