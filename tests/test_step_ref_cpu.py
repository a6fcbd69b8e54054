"""
tests/step_ref.py without a GPU: the restatement against oracle/sampler_ref and the written-out torch DDIM expression,
bit for bit; the step tests' comparator against nine mutants of the restatement on the step tests' own inputs, each
of which it has to see; and the host check of t in p_sample / ddim_sample, which has to refuse before the model runs.
"""

import numpy as np
import pytest
import torch

import step_ref as SR
from guided_diffusion import script_util as su
from oracle import sampler_ref

F = np.float32


@pytest.fixture(scope="module")
def runs():
    """every launch of every case with its unmutated restatement, computed once and left unchanged"""
    return [(case, label, kw, SR.step(**kw)) for case in SR.CASES for label, kw in SR.launches(case)]


def test_cases_cover_the_axes():
    names = [c["name"] for c in SR.CASES]
    assert len(names) == len(set(names))
    for kind in ("ddpm", "ddim"):
        mine = [c for c in SR.CASES if c["kind"] == kind]
        flags = {(c["learn"], c["px"], c["clip"]) for c in mine if c["variant"] == "plain" and not c["poison"]}
        assert flags == set(SR.FLAGS)
        assert {c["voxels"] for c in mine} == {1, 255, 257, SR.STRIDE + 257}
        assert {c["respacing"] for c in mine} == {"10", ""}
        assert any(c["sigma_small"] for c in mine) and any(c["variant"] == "x0" for c in mine)
        assert {c["clip"] for c in mine if c["poison"]} == {True, False}
    assert {e for c in SR.CASES if c["kind"] == "ddim" for e in c["etas"]} == {0.0, 0.7, 1.0}


def test_a_third_of_x0_lies_outside_the_clip(runs):
    """Both sides of the clip are populated in every launch.  Launches of fewer than 255 values are left out of this
    one assertion: the share of three values is a multiple of a third."""
    for case, label, kw, ref in runs:
        if kw["x"].size < 255:
            continue
        share = SR.share_of(kw)
        assert 0.10 <= share <= 0.60, (label, share)


def _torch(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _sqrt(v):
    """The correctly rounded fp32 square root, which is what np.sqrt and the device's sqrtf return: the fp64 root
    rounded once (53 >= 2 * 24 + 2 bits, so the double rounding is exact).  torch.sqrt on fp32 CPU tensors is not
    correctly rounded on every host: for 4.1181935e-05 (alphas_cumprod_prev[999] of linear-1000), whose root
    0.006417315221... lies 0.498 / 0.502 ulp from its two fp32 neighbours, it returns the farther one."""
    return torch.sqrt(v.double()).float()


def test_restatement_equals_the_oracle_bit_for_bit(runs):
    """mean, log_variance and pred_xstart against oracle/sampler_ref.mean_variance (one call per sample: it takes one
    step index per batch), the DDPM sample within the step tests' bar of mean + mask exp(0.5 logvar) z, the DDIM
    sample against the torch expression tests/test_gpu_ops.py::test_sampler_update_kernels writes out, its four
    square roots taken through _sqrt.  The _x0 launches are the oracle under predict_xstart with the finished x0 as
    the model output's first half."""
    for case, label, kw, ref in runs:
        tb = SR.schedule(kw["respacing"])
        mo, px = kw["mo"], kw["predict_xstart"]
        if kw["xstart"] is not None:
            mo, px = mo.copy(), True
            mo[:, 0] = kw["xstart"]
        sample = np.empty_like(ref["sample"])
        for n, i in enumerate(kw["t"]):
            x, z = _torch(kw["x"][n][None, None]), _torch(kw["z"][n][None, None])
            mean, logvar, x0 = sampler_ref.mean_variance(tb, _torch(mo[n][None]), x, i, kw["learn_sigma"], px,
                                                         kw["clip"], kw["sigma_small"])
            for name, a in (("mean", mean), ("log_variance", logvar), ("pred_xstart", x0)):
                assert SR.compare(a.numpy()[0, 0], ref[name][n]) == 0, (label, n, name)
            mask = 0.0 if i == 0 else 1.0
            if kw["kind"] == "ddpm":
                sample[n] = (mean + mask * torch.exp(0.5 * logvar) * z).numpy()[0, 0]
            else:
                c = lambda k: float(np.float32(tb[k][i]))
                eps = (c("sqrt_recip_alphas_cumprod") * x - x0) / c("sqrt_recipm1_alphas_cumprod")
                ab, abp = torch.tensor(c("alphas_cumprod")), torch.tensor(c("alphas_cumprod_prev"))
                sig = kw["eta"] * _sqrt((1 - abp) / (1 - ab)) * _sqrt(1 - ab / abp)
                ref2 = x0 * _sqrt(abp) + _sqrt(1 - abp - sig ** 2) * eps + mask * sig * z
                sample[n] = ref2.numpy()[0, 0]
        assert SR.check(kw["kind"], sample, ref["pred_xstart"], ref, kw["t"]) == {}, label


def test_nan_and_inf_pass_through_the_restatement_as_through_torch(runs):
    """what the non-finite cases rely on: NaN in eps stays NaN through the clip, +-Inf in eps clips to -+1"""
    for case, label, kw, ref in runs:
        if "mo" not in label.split("-") or not kw["clip"]:
            continue
        e = kw["mo"][:, 0]
        x0 = ref["pred_xstart"]
        assert np.isnan(e).any() and np.isnan(x0[np.isnan(e)]).all(), label
        assert (x0[e == np.inf] == -1).all() and (x0[e == -np.inf] == 1).all(), label


# ---------------------------------------------------------------------------------------------------------- mutants
class RowOfSampleZero(SR.Ops):
    """1. t_idx[0] used for all samples"""
    def rows(self, t):
        return np.full_like(t, t[0])


class MaskOfSampleZero(SR.Ops):
    """2. noise mask taken from sample 0"""
    def mask_rows(self, rows):
        return np.full_like(rows, rows[0])


class FusedPosteriorMean(SR.Ops):
    """3. c1 * x0 + c2 * x contracted to one FMA: the first product exact (fp64 holds it), one rounding of the sum"""
    def posterior_mean(self, c1, x0, c2, x):
        return (c1.astype(np.float64) * x0.astype(np.float64) + (c2 * x).astype(np.float64)).astype(F)


class RatioReordered(SR.Ops):
    """4. 1 - ab / ab_prev computed as (ab_prev - ab) / ab_prev"""
    def one_minus_ratio(self, ab, ab_prev):
        return (ab_prev - ab) / ab_prev


class SecondHalfOfTheNextRow(SR.Ops):
    """5. second-half index (n * ch + 1) replaced by (n + 1)"""
    def variance_half(self, mo, n):
        return mo.reshape(-1, mo.shape[-1])[n + 1]


class FminFmaxClip(SR.Ops):
    """8. fmaxf / fminf clip semantics: NaN becomes -1"""
    def clip(self, x0):
        return np.fmin(np.fmax(x0, F(-1)), F(1))


class EtaIgnoredInTheDirection(SR.Ops):
    """9. eta ignored in sqrt(1 - ab_prev - sigma^2)"""
    def direction(self, ab_prev, sigma):
        return np.sqrt(F(1) - ab_prev)


def _with(ops):
    return lambda kw: SR.step(ops=ops(), **kw)


def _tail_unwritten(kw):
    """6. the last voxels % 256 elements left unwritten: the outputs keep the NaN they were filled with"""
    r = SR.step(**kw)
    tail = kw["x"].shape[1] % 256
    if tail:
        r["sample"][:, -tail:] = np.nan
        r["pred_xstart"][:, -tail:] = np.nan
    return r


def _second_pass_reads_the_first(kw):
    """7. the second grid pass reading x[v - stride]"""
    x = kw["x"].copy()
    x[:, SR.STRIDE:] = kw["x"][:, :max(x.shape[1] - SR.STRIDE, 0)]
    return SR.step(**dict(kw, x=x))


MUTANTS = {
    "1-row-of-sample-zero": _with(RowOfSampleZero),
    "2-mask-of-sample-zero": _with(MaskOfSampleZero),
    "3-fused-posterior-mean": _with(FusedPosteriorMean),
    "4-ratio-reordered": _with(RatioReordered),
    "5-second-half-of-the-next-row": _with(SecondHalfOfTheNextRow),
    "6-tail-unwritten": _tail_unwritten,
    "7-second-pass-reads-the-first": _second_pass_reads_the_first,
    "8-fmin-fmax-clip": _with(FminFmaxClip),
    "9-eta-ignored-in-the-direction": _with(EtaIgnoredInTheDirection),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_comparator_sees_every_mutant(runs, name):
    """The GPU test's comparator on the GPU test's inputs, mutant against the unmutated restatement: at least one
    launch has to fail, or the inputs or the bars are too weak to see that error in a kernel."""
    seen = []
    for case, label, kw, ref in runs:
        m = MUTANTS[name](kw)
        fails = SR.check(kw["kind"], m["sample"], m["pred_xstart"], ref, kw["t"])
        if fails:
            seen.append((label, fails))
    print("%s: seen in %d of %d launches, e.g. %s" % (name, len(seen), len(runs), seen[:3]))
    assert seen, name


def test_the_comparator_passes_the_restatement_itself(runs):
    for case, label, kw, ref in runs:
        again = SR.step(**kw)
        assert SR.check(kw["kind"], again["sample"], again["pred_xstart"], ref, kw["t"]) == {}, label


# ------------------------------------------------------------------------------------------------ t is checked first
class Reached(Exception):
    pass


@pytest.mark.parametrize("call", ["p_sample", "ddim_sample"])
def test_a_bad_t_is_refused_before_the_model_runs(call):
    """The step kernel behind p_sample and ddim_sample takes no T: a t outside [0, T) would be a read past the
    coefficient table, so it never gets as far as a launch (the reference raises IndexError for it)."""
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="10")
    T = d.num_timesteps
    calls = []

    def model(x, t, **kw):
        calls.append(t)
        raise Reached()

    x = torch.zeros(1, 1, 4, 4, 4)
    fn = getattr(d, call)
    for bad in (torch.tensor([T]), torch.tensor([-1]), torch.tensor([3.0]), torch.tensor([3, 3]), [T]):
        with pytest.raises(ValueError):
            fn(model, x, bad)
    assert calls == []
    # a t inside the range gets through to the model
    with pytest.raises(Reached):
        fn(model, x, torch.tensor([T - 1]))
    assert len(calls) == 1
