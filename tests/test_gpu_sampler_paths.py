"""
The bits of every host path around the step kernels: each loop (DDPM, DDIM, DPM-Solver++, DDIM
inversion), the single-step calls and the joint loop, with tensor noise and with a NoiseKey, without a guide and with a
LowPassPull whose stop_t falls inside the schedule, each under a StepTrace.  The SHA-256 of every step's sample and
pred_xstart and of the trace's records is compared to tests/golden/sampler_paths.json, which was recorded once on an
MI355X from a trusted build (its header names the commit):

    python tests/test_gpu_sampler_paths.py --record COMMIT      # in a checkout of that commit; writes the golden

The network is a callable of exact fp32 multiplies and adds, one torch op each, and every noise tensor is numpy-seeded
or keyed, so the bits depend on this package's kernels and host code alone.  Shape (2, 1, 4, 6, 10): two samples (the
per-sample t row, the grid's sample axis) of 240 voxels, ragged against the 256-thread workgroup.

The stochastic solver exists for orders 1 and 2 (order 3 is refused by _check_solver, asserted below), so those are
the stochastic cases.  Runs that draw from torch's generator are not recorded: they are pinned to the same loop fed
the same draws explicitly, which fixes the draw order whatever the torch build.
"""

import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from guided_diffusion import gaussian_diffusion as gd
from guided_diffusion import guidance, joint, metrics, patches
from guided_diffusion import script_util as su

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "sampler_paths.json")
SHAPE = (2, 1, 4, 6, 10)
STEPS = 6
SCHEDULES = {"spaced6": dict(steps=1000, learn_sigma=True, timestep_respacing="6"),
             "plain6": dict(steps=STEPS, learn_sigma=False, noise_schedule="cosine")}
# loop tag -> (kind, arguments of its loop, whether every step reads noise)
LOOPS = {"ddpm": ("ddpm", {}, True), "ddim_eta0": ("ddim", dict(eta=0.0), True),
         "ddim_eta0.5": ("ddim", dict(eta=0.5), True),
         "ode1": ("solver", dict(order=1), False), "ode2": ("solver", dict(order=2), False),
         "ode3": ("solver", dict(order=3), False),
         "sde1": ("solver", dict(order=1, stochastic=True), True),
         "sde2": ("solver", dict(order=2, stochastic=True), True)}
JOINT_SHAPE, JOINT_RES = (20, 40, 40), 16          # test_gpu_joint.py's smallest geometry


class Affine:
    """model(x, t, low_res) of single fp32 products and sums: [0.3 x + 0.7 low_res, -0.4 x] (the second half only
    under learn_sigma)"""

    def __init__(self, learn_sigma):
        self.learn_sigma = learn_sigma

    def __call__(self, x, t, low_res):
        a = x * 0.3
        b = low_res * 0.7
        m = a + b
        return torch.cat([m, x * -0.4], 1) if self.learn_sigma else m


def normals(seed, shape=SHAPE):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()


def sha(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def setup(schedule):
    diff = su.create_gaussian_diffusion(**SCHEDULES[schedule])
    assert diff.num_timesteps == STEPS
    return diff, Affine(SCHEDULES[schedule]["learn_sigma"]), {"low_res": normals(3)}


def pull(diff):
    """active on the upper half of the schedule only"""
    g = guidance.LowPassPull(4.0, (2.0, 2.0, 2.0), weight=0.5, stop_t=int(diff.timestep_map[3]))
    assert [g.active(diff, i) for i in range(STEPS)] == [False] * 3 + [True] * 3
    return g


def noise_args(source, per_step):
    if source == "key":
        return dict(noise_key=gd.NoiseKey(1234, [7, 11], device="cuda:0"))
    kw = dict(noise=normals(10))
    if per_step:
        kw["step_noise"] = [normals(11 + k) for k in range(STEPS)]
    return kw


def steps_of(gen, trace=None):
    out = {"steps": [[sha(r["sample"]), sha(r["pred_xstart"])] for r in gen]}
    if trace is not None:
        out["trace"] = sha(trace.records())
        out["trace_t"] = [int(v) for v in trace.t]
    return out


def run_loop(schedule, tag, source, guided):
    diff, model, kw = setup(schedule)
    kind, args, per_step = LOOPS[tag]
    trace = metrics.StepTrace(target=normals(4))
    fn = {"ddpm": diff.p_sample_loop_progressive, "ddim": diff.ddim_sample_loop_progressive,
          "solver": diff.dpm_solver_sample_loop_progressive}[kind]
    return steps_of(fn(model, SHAPE, model_kwargs=kw, device="cuda:0", trace=trace, guide=pull(diff) if guided else None,
                       **noise_args(source, per_step), **args), trace)


def run_inversion(schedule):
    diff, model, kw = setup(schedule)
    trace = metrics.StepTrace(target=normals(4))
    return steps_of(diff.ddim_reverse_sample_loop_progressive(model, normals(5), model_kwargs=kw, trace=trace), trace)


def run_single(schedule, kind, source, guided):
    diff, model, kw = setup(schedule)
    t = torch.tensor([5, 4], device="cuda:0")         # one row of the table per sample, both on the guide's active side
    noise = dict(noise_key=gd.NoiseKey(1234, [7, 11], device="cuda:0"), draw=3) if source == "key" else \
        dict(noise=normals(12))
    fn, args = (diff.p_sample, {}) if kind == "ddpm" else (diff.ddim_sample, dict(eta=0.5))
    return steps_of([fn(model, normals(5), t, model_kwargs=kw, guide=pull(diff) if guided else None, **noise, **args)])


def run_joint(source):
    diff, _, _ = setup("spaced6")
    geom = patches.joint_geometry(JOINT_SHAPE, JOINT_RES)
    low = np.random.default_rng(6).standard_normal(JOINT_SHAPE).astype(np.float32)
    noise = dict(noise_key=joint.draw_key(99, 1, device="cuda:0")) if source == "key" else {}
    return steps_of(joint.sample_loop_progressive(diff, Affine(True), low, geom, batch_size=5, device="cuda:0", **noise))


def cases():
    c = {}
    for schedule in SCHEDULES:
        for tag in LOOPS:
            for source in ("tensor", "key"):
                for guided in (False, True):
                    name = "%s/%s/%s/%s" % (schedule, tag, source, "pull" if guided else "plain")
                    c[name] = (run_loop, schedule, tag, source, guided)
        c["%s/inversion" % schedule] = (run_inversion, schedule)
        for kind in ("ddpm", "ddim"):
            for source in ("tensor", "key"):
                for guided in (False, True):
                    name = "%s/single_%s/%s/%s" % (schedule, kind, source, "pull" if guided else "plain")
                    c[name] = (run_single, schedule, kind, source, guided)
    c["joint/generator"] = (run_joint, "generator")
    c["joint/key"] = (run_joint, "key")
    return c


CASES = cases()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_FILE) as f:
        g = json.load(f)
    assert sorted(g["cases"]) == sorted(CASES)
    return g["cases"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_bits_are_the_recorded_ones(recorded, case):
    fn, *args = CASES[case]
    assert fn(*args) == recorded[case], case


@pytest.mark.parametrize("tag", ["ddpm", "ddim_eta0.5", "sde2"])
def test_default_noise_is_randn_then_one_randn_like_per_step(tag):
    """x_T = th.randn, then exactly one randn_like per step, in that order: the seeded default run equals the run fed
    those draws as noise= and step_noise=."""
    diff, model, kw = setup("spaced6")
    kind, args, _ = LOOPS[tag]
    fn = {"ddpm": diff.p_sample_loop_progressive, "ddim": diff.ddim_sample_loop_progressive,
          "solver": diff.dpm_solver_sample_loop_progressive}[kind]
    torch.manual_seed(5)
    default = steps_of(fn(model, SHAPE, model_kwargs=kw, device="cuda:0", **args))
    torch.manual_seed(5)
    x_T = torch.randn(*SHAPE, device="cuda:0")
    draws = [torch.randn_like(x_T) for _ in range(STEPS)]
    assert steps_of(fn(model, SHAPE, noise=x_T, step_noise=draws, model_kwargs=kw, device="cuda:0", **args)) == default


def test_where_the_refusals_surface():
    """The solver's loop is a plain function that checks at the call; the other loops are generators whose argument
    errors surface at the first next()."""
    diff, model, kw = setup("spaced6")
    with pytest.raises(ValueError, match="order must be 1, 2 or 3"):
        diff.dpm_solver_sample_loop_progressive(model, SHAPE, model_kwargs=kw, device="cuda:0", order=4)
    with pytest.raises(ValueError, match="orders 1 and 2 only"):
        diff.dpm_solver_sample_loop_progressive(model, SHAPE, model_kwargs=kw, device="cuda:0", order=3,
                                                stochastic=True)
    with pytest.raises(RuntimeError, match="sampling runs on HIP kernels only"):
        diff.dpm_solver_sample_loop_progressive(model, SHAPE, model_kwargs=kw, device="cpu")
    gen = diff.p_sample_loop_progressive(model, SHAPE, model_kwargs=kw, device="cpu")
    with pytest.raises(RuntimeError, match="sampling runs on HIP kernels only"):
        next(gen)
    gen = diff.ddim_reverse_sample_loop_progressive(model, normals(5), model_kwargs=kw, device="cpu")
    with pytest.raises(RuntimeError, match="DDIM inversion runs on HIP kernels only"):
        next(gen)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_sampler_paths.py --record COMMIT   (in a checkout of that commit)")
    header = "SHA-256 per step of [sample, pred_xstart] and of the trace records; recorded on an MI355X (gfx950) " \
             "from a build of commit %s" % sys.argv[2]
    with open(GOLDEN_FILE, "w") as f:
        json.dump({"header": header, "cases": {name: c[0](*c[1:]) for name, c in sorted(CASES.items())}}, f, indent=0,
                  sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases)" % (GOLDEN_FILE, len(CASES)))
