#!/usr/bin/env python3
"""
Generate tests/golden/bpd.npz by RUNNING THE REFERENCE's variational-bound code (gaussian_diffusion.py:171-230,
:709-742, :821-894; losses.py) on seeded synthetic inputs:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bpd.py

Build container only, like make_golden.py, whose helpers (flags, load_synth, _InjectNoise, synth) it reuses.
Stored: the reference's OUTPUTS and the seeds of the inputs; the inputs themselves are regenerated on both sides
from guided_diffusion/synth.py's numpy recipes (synth_x_start, synth_model_output, synth_noise, synth_low_res).

Kernel level ("k/..."): _vb_terms_bpd with a model that returns a fixed, seeded output (the trick
training_losses uses at :792), for N = 3 volumes of 16x32x32 at t = [0, T/2, T-1] of the "250" schedule; the
x_0 and eps MSEs as calc_bpd_loop forms them (:877-880); q_sample and _prior_bpd of the same batch.
End to end ("e/..."): calc_bpd_loop on seeded networks with the per-step randn_like draws injected.
"""

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden import PUBLISHED, TINY, _InjectNoise, flags, load_synth, ref_su, synth  # noqa: E402
from guided_diffusion import nn as ref_nn  # noqa: E402  (the reference's, imported by make_golden)

SEEDS = dict(x_start=21, noise=22, model_output=23, low_res=1234, steps=10)
K_SHAPE = (3, 1, 16, 32, 32)
K_RESPACING = "250"
K_VARIANTS = {                 # tag: create_gaussian_diffusion flags
    "learned_range": dict(learn_sigma=True),
    "fixed_large": dict(learn_sigma=False),
    "xstart": dict(learn_sigma=True, predict_xstart=True),
}
E_CASES = [                    # tag, model flags, shape, calc_bpd_loop kwargs
    ("tiny10", TINY, (2, 1, 8, 16, 16), {}),
    ("tiny10_nosigma", dict(TINY, learn_sigma=False), (1, 1, 4, 16, 16), {}),
    ("tiny10_noclip", TINY, (1, 1, 4, 16, 16), dict(clip_denoised=False)),
    ("tiny10_xstart", dict(TINY, predict_xstart=True), (1, 1, 4, 16, 16), {}),
    ("published10", PUBLISHED, (1, 1, 8, 32, 32), {}),
]
OUTPUTS = ["total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"]


def kernel_cases(out):
    x_start = torch.from_numpy(synth.synth_x_start(K_SHAPE, SEEDS["x_start"]))
    noise = torch.from_numpy(synth.synth_noise(K_SHAPE, 1, seed=SEEDS["noise"])[0])
    base = ref_su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing=K_RESPACING)
    T = base.num_timesteps
    t = torch.tensor([0, T // 2, T - 1])
    out["k/t"] = t.numpy()
    x_t = base.q_sample(x_start, t, noise=noise)
    out["k/q_sample"] = x_t.numpy()
    out["k/prior_bpd"] = base._prior_bpd(x_start).numpy()
    for tag, over in K_VARIANTS.items():
        d = ref_su.create_gaussian_diffusion(steps=1000, timestep_respacing=K_RESPACING, **over)
        mo = torch.from_numpy(synth.synth_model_output(K_SHAPE, over["learn_sigma"], SEEDS["model_output"]))
        for clip in (True, False):
            key = "k/%s/%s" % (tag, "clip" if clip else "noclip")
            with torch.no_grad():
                r = d._vb_terms_bpd(lambda *a, r=mo: r, x_start, x_t, t, clip_denoised=clip)
                px = r["pred_xstart"]
                eps = d._predict_eps_from_xstart(x_t, t, px)
            out[key + "/vb"] = r["output"].numpy()
            out[key + "/xstart_mse"] = ref_nn.mean_flat((px - x_start) ** 2).numpy()
            out[key + "/mse"] = ref_nn.mean_flat((eps - noise) ** 2).numpy()
            print(key, out[key + "/vb"], out[key + "/xstart_mse"], out[key + "/mse"])


def end_to_end(out):
    for tag, fl, shape, kw in E_CASES:
        t0 = time.time()
        model, diff = ref_su.sr_create_model_and_diffusion(**flags(**dict(fl, timestep_respacing="10")))
        load_synth(model)
        T = diff.num_timesteps
        draws = synth.synth_noise(shape, T, seed=SEEDS["steps"])
        x_start = torch.from_numpy(synth.synth_x_start(shape, SEEDS["x_start"]))
        lr = torch.from_numpy(synth.synth_low_res(shape, seed=SEEDS["low_res"]))
        with _InjectNoise(draws), torch.no_grad():
            r = diff.calc_bpd_loop(model, x_start, model_kwargs={"low_res": lr}, **kw)
        for k in OUTPUTS:
            out["e/%s/%s" % (tag, k)] = r[k].numpy()
        print(tag, "total_bpd", r["total_bpd"].numpy(), "%.0f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    res = {"seeds": np.array([SEEDS[k] for k in ("x_start", "noise", "model_output", "low_res", "steps")],
                             dtype=np.int64)}
    kernel_cases(res)
    end_to_end(res)
    np.savez_compressed(os.path.join(HERE, "bpd.npz"), **res)
    print("wrote bpd.npz", len(res), "arrays")
