#!/usr/bin/env python3
"""
ODE-solution error of the DPM-Solver++ multistep sampler against DDIM on the published network (seeded synthetic
weights, 1 x 64^3, the default f16x3 mode, clip_denoised=False), one process, one device.

Reference solution: 3M on "logsnr500" from a fixed x_T; DDIM on the full 1000-step schedule from the same x_T is
run too and its disagreement with the reference reported as the reference's own error.  Then DDIM (ddim_sample_loop,
eta = 0), 2M and 3M for N in --steps on both "ddimN" and "logsnrN" spacing, each reported as max |x - ref| / max |ref|
and as the RMS ratio.  Last, ms per step of dpm_solver_sample_loop (order 2) against ddim_sample_loop on the same
schedule (host clock around a whole loop ending in a device synchronise, best of --reps).  Prints one JSON line.

    python tools/solver_quality.py [--steps 10,15,20,25,50] [--size 64] [--reps 3] [--out q.json]
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-denoising-diffusion-model_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from guided_diffusion import script_util as su  # noqa: E402
from guided_diffusion import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="10,15,20,25,50")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--ref_steps", type=int, default=500)
    ap.add_argument("--time_respacing", default="logsnr20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("solver_quality: no GPU visible (there is nothing to measure on the host)")
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(bench.PUBLISHED, "", dev)
    shape = (1, 1, a.size, a.size, a.size)
    x_T = torch.from_numpy(synth.synth_noise(shape, 1, seed=10)[0]).to(dev)
    kw = {"low_res": torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)}
    diffs = {}

    def diffusion(resp):
        if resp not in diffs:
            diffs[resp] = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing=resp)
        return diffs[resp]

    def run(resp, solver):
        d = diffusion(resp)
        if solver == "ddim":
            return d.ddim_sample_loop(model, shape, x_T.clone(), clip_denoised=False, model_kwargs=kw, eta=0.0)
        return d.dpm_solver_sample_loop(model, shape, x_T.clone(), clip_denoised=False, model_kwargs=kw,
                                        order=int(solver[0]))

    def errors(x, ref):
        dx = (x.double() - ref.double())
        return {"max_rel": float(dx.abs().max() / ref.double().abs().max()),
                "rms_rel": float(dx.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())}

    t0 = time.perf_counter()
    ref = run("logsnr%d" % a.ref_steps, "3m")
    ddim_full = run("", "ddim")
    res = {
        "what": "relative error of the final sample against 3M on logsnr%d from the same x_T (ODE form, "
                "clip_denoised=False), and ms per step" % a.ref_steps,
        "network": "published (SuperResModel_noatt, 128 ch, mult (1,1,2,3,4)), seeded synthetic weights",
        "shape": list(shape), "precision": model.conv_precision, "device": torch.cuda.get_device_name(dev),
        "reference": "3m logsnr%d" % a.ref_steps,
        "reference_vs_ddim1000": errors(ddim_full, ref),
        "errors": {},
    }
    for n in (int(v) for v in a.steps.split(",")):
        for spacing in ("ddim", "logsnr"):
            resp = "%s%d" % (spacing, n)
            res["errors"][resp] = {solver: errors(run(resp, solver), ref) for solver in ("ddim", "2m", "3m")}
    res["quality_wall_s"] = time.perf_counter() - t0

    d = diffusion(a.time_respacing)
    T = d.num_timesteps

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / T

    def dpm():
        return d.dpm_solver_sample_loop(model, shape, x_T.clone(), model_kwargs=kw, order=2)

    def ddim():
        return d.ddim_sample_loop(model, shape, x_T.clone(), model_kwargs=kw, eta=0.0)

    timed(dpm)
    timed(ddim)
    ms = {"dpm_solver_2m": [], "ddim": []}
    for _ in range(a.reps):
        ms["dpm_solver_2m"].append(timed(dpm))
        ms["ddim"].append(timed(ddim))
    res["time"] = {"respacing": a.time_respacing, "steps": T,
                   "dpm_solver_sample_loop_ms_per_step": min(ms["dpm_solver_2m"]),
                   "ddim_sample_loop_ms_per_step": min(ms["ddim"]),
                   "ratio_min": min(ms["dpm_solver_2m"]) / min(ms["ddim"]), "all_ms_per_step": ms}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
