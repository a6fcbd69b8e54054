#!/usr/bin/env python3
"""
Generate tests/golden/guidance.npz by RUNNING THE REFERENCE's p_sample and ddim_sample (gaussian_diffusion.py:395-439,
:537-585) with denoised_fn = the low-pass pull of tests/guidance_ref.py, on seeded synthetic inputs:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_guidance.py

Build container only, like make_golden.py, whose helpers it reuses as make_golden_ddim_reverse.py does.  Stored: the
reference's OUTPUTS and the seeds of the inputs; the inputs are regenerated on both sides from
guided_diffusion/synth.py's numpy recipes, the taps from guidance_ref.taps_for.

A model that returns a fixed, seeded output, N = 3 volumes of 4x16x16 at t = [0, T/2, T-1] of the "250" schedule, the
four variance / mean variants of make_golden_ddim_reverse.py with and without the clip, the radii (1, 2, 3) and
(0, 0, 0) along (D, H, W), weight 0.75.  Per case: pred_xstart (the same for all three calls, asserted) and the
samples of p_sample, ddim_sample(eta=0) and ddim_sample(eta=0.5), all with the same injected noise.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _InjectNoise, ref_su, synth  # noqa: E402
from make_golden_ddim_reverse import K_RESPACING, K_SHAPE, K_VARIANTS  # noqa: E402
import guidance_ref  # noqa: E402

SEEDS = dict(x=22, model_output=23, measurement=77, noise=78)
RADII = {"r123": (1, 2, 3), "r000": (0, 0, 0)}
WEIGHT = 0.75
ETAS = (0.0, 0.5)


def cases(out):
    x = torch.from_numpy(synth.synth_noise(K_SHAPE, 1, seed=SEEDS["x"])[0])
    y = torch.from_numpy(synth.synth_low_res(K_SHAPE, seed=SEEDS["measurement"]))
    z = synth.synth_noise(K_SHAPE, 1, seed=SEEDS["noise"])[0]
    base = ref_su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing=K_RESPACING)
    T = base.num_timesteps
    t = torch.tensor([0, T // 2, T - 1])
    out["t"] = t.numpy()
    for tag, over in K_VARIANTS.items():
        d = ref_su.create_gaussian_diffusion(steps=1000, timestep_respacing=K_RESPACING, **over)
        mo = torch.from_numpy(synth.synth_model_output(K_SHAPE, over["learn_sigma"], SEEDS["model_output"]))
        model = lambda *a, r=mo: r  # noqa: E731
        for rtag, radii in RADII.items():
            taps = guidance_ref.taps_for(radii)
            fn = lambda x0: guidance_ref.pull(x0, y, taps, WEIGHT)  # noqa: E731
            for clip in (True, False):
                key = "%s/%s/%s" % (tag, rtag, "clip" if clip else "noclip")
                with torch.no_grad():
                    with _InjectNoise([z]):
                        p = d.p_sample(model, x, t, clip_denoised=clip, denoised_fn=fn)
                    out[key + "/pred_xstart"] = p["pred_xstart"].numpy()
                    out[key + "/p_sample"] = p["sample"].numpy()
                    for eta in ETAS:
                        with _InjectNoise([z]):
                            r = d.ddim_sample(model, x, t, clip_denoised=clip, denoised_fn=fn, eta=eta)
                        assert torch.equal(r["pred_xstart"], p["pred_xstart"])
                        out[key + "/ddim_eta%g" % eta] = r["sample"].numpy()
                print(key, float(p["sample"].abs().max()), float(p["pred_xstart"].abs().max()), flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    res = {"seeds": np.array([SEEDS[k] for k in ("x", "model_output", "measurement", "noise")], dtype=np.int64),
           "weight": np.float32(WEIGHT)}
    cases(res)
    np.savez_compressed(os.path.join(HERE, "guidance.npz"), **res)
    print("wrote guidance.npz", len(res), "arrays")
