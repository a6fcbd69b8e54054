#!/usr/bin/env python3
"""
Generate tests/golden/ddim_reverse.npz by RUNNING THE REFERENCE's p_mean_variance and ddim_reverse_sample
(gaussian_diffusion.py:232-326, :587-623) on seeded synthetic inputs:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ddim_reverse.py

Build container only, like make_golden.py, whose helpers (flags, load_synth, synth) it reuses as make_golden_bpd.py
does.  Stored: the reference's OUTPUTS and the seeds of the inputs; the inputs themselves are regenerated on both
sides from guided_diffusion/synth.py's numpy recipes (synth_noise, synth_model_output, synth_x_start, synth_low_res).

Kernel level ("k/..."): both calls with a model that returns a fixed, seeded output (the trick training_losses uses
at :792), for N = 3 volumes of 4x16x16 at t = [0, T/2, T-1] of the "250" schedule.  Under the fixed variance types
the variance and log-variance are per-sample constants: their [N] values are stored.
End to end ("e/..."): DDIM inversion written out over the reference's ddim_reverse_sample -- from x = x_start,
x <- ddim_reverse_sample(x, t=k)["sample"] for k = 0 ... T-1 -- on seeded networks with "ddim10".  Every step's
sample for the tiny networks; the final sample and the last pred_xstart for the published one.
"""

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden import PUBLISHED, TINY, flags, load_synth, ref_su, synth  # noqa: E402

SEEDS = dict(x=22, model_output=23, x_start=21, low_res=1234)
K_SHAPE = (3, 1, 4, 16, 16)
K_RESPACING = "250"
K_VARIANTS = {                 # tag: create_gaussian_diffusion flags
    "learned_range": dict(learn_sigma=True),
    "fixed_large": dict(learn_sigma=False),
    "fixed_small": dict(learn_sigma=False, sigma_small=True),
    "xstart": dict(learn_sigma=True, predict_xstart=True),
}
E_RESPACING = "ddim10"
E_CASES = [                    # tag, model flags, shape, loop kwargs
    ("tiny", TINY, (2, 1, 4, 16, 16), {}),
    ("tiny_noclip", TINY, (1, 1, 4, 16, 16), dict(clip_denoised=False)),
    ("tiny_nosigma", dict(TINY, learn_sigma=False), (1, 1, 4, 16, 16), {}),
    ("tiny_xstart", dict(TINY, predict_xstart=True), (1, 1, 4, 16, 16), {}),
    ("published", PUBLISHED, (1, 1, 8, 32, 32), {}),
]


def kernel_cases(out):
    x = torch.from_numpy(synth.synth_noise(K_SHAPE, 1, seed=SEEDS["x"])[0])
    base = ref_su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing=K_RESPACING)
    T = base.num_timesteps
    t = torch.tensor([0, T // 2, T - 1])
    out["k/t"] = t.numpy()
    for tag, over in K_VARIANTS.items():
        d = ref_su.create_gaussian_diffusion(steps=1000, timestep_respacing=K_RESPACING, **over)
        learn = over["learn_sigma"]
        mo = torch.from_numpy(synth.synth_model_output(K_SHAPE, learn, SEEDS["model_output"]))
        for clip in (True, False):
            key = "k/%s/%s" % (tag, "clip" if clip else "noclip")
            with torch.no_grad():
                pmv = d.p_mean_variance(lambda *a, r=mo: r, x, t, clip_denoised=clip)
                rev = d.ddim_reverse_sample(lambda *a, r=mo: r, x, t, clip_denoised=clip)
            assert torch.equal(pmv["pred_xstart"], rev["pred_xstart"])
            out[key + "/mean"] = pmv["mean"].numpy()
            out[key + "/pred_xstart"] = pmv["pred_xstart"].numpy()
            out[key + "/sample"] = rev["sample"].numpy()
            for k in ("variance", "log_variance"):
                v = pmv[k].contiguous().numpy()
                out[key + "/" + k] = v if learn else v.reshape(v.shape[0], -1)[:, 0].copy()
            print(key, float(rev["sample"].abs().max()), float(pmv["log_variance"].mean()))


def end_to_end(out):
    for tag, fl, shape, kw in E_CASES:
        t0 = time.time()
        model, diff = ref_su.sr_create_model_and_diffusion(**flags(**dict(fl, timestep_respacing=E_RESPACING)))
        load_synth(model)
        T = diff.num_timesteps
        x = torch.from_numpy(synth.synth_x_start(shape, SEEDS["x_start"]))
        lr = torch.from_numpy(synth.synth_low_res(shape, seed=SEEDS["low_res"]))
        steps = []
        with torch.no_grad():
            for k in range(T):
                r = diff.ddim_reverse_sample(model, x, torch.tensor([k] * shape[0]), model_kwargs={"low_res": lr},
                                             **kw)
                x = r["sample"]
                steps.append(x.numpy())
        if tag == "published":
            out["e/%s/sample" % tag] = steps[-1]
            out["e/%s/pred_xstart" % tag] = r["pred_xstart"].numpy()
        else:
            out["e/%s/samples" % tag] = np.stack(steps)
        print(tag, "x_T std %.4f" % float(x.std()), "%.0f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    res = {"seeds": np.array([SEEDS[k] for k in ("x", "model_output", "x_start", "low_res")], dtype=np.int64)}
    kernel_cases(res)
    end_to_end(res)
    np.savez_compressed(os.path.join(HERE, "ddim_reverse.npz"), **res)
    print("wrote ddim_reverse.npz", len(res), "arrays")
