#!/usr/bin/env python3
"""
What the low-pass data-consistency guidance costs, one process, one device.  Every comparison is
against the un-guided path of the same run, alternated with it; every row carries the scatter (max - min over the
reps) of both.

pull     ddpm3d_xstart_pull at 1 x 96^3 and 8 x 96^3, for radius 0 (the pointwise pull) and for the radii of an 8 mm
         FWHM on 2 mm voxels: device-event ms and GB/s of its nominal traffic, 16 bytes per voxel (model output's
         first half, x, measurement read, x0 written) plus 8 per voxel for every pass after the first (one volume
         written, one read).
step     the pull followed by ddpm3d_p_sample_step_x0 beside the un-guided ddpm3d_p_sample_step, at the same shapes.
loop     p_sample_loop of the published network at 1 x 96^3 with and without guide=: host clock around a whole loop
         ending in a device synchronise, ms per step, as pairs alternated over the reps.

    python tools/guidance_time.py [--reps 5] [--inner 10] [--respacing 10] [--json profiles/guidance_time.json]
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-denoising-diffusion-model_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from guided_diffusion import _hip as H  # noqa: E402
from guided_diffusion import guidance, synth  # noqa: E402
from guided_diffusion import script_util as su  # noqa: E402
from noise_time import alternated, host_timed, summary  # noqa: E402

DHW = (96, 96, 96)
PULLS = [("radius 0", 0.0), ("8 mm FWHM on 2 mm voxels", 8.0)]


def kernel_rows(args, dev):
    lib = H.load()
    diff = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="10")
    coef = diff._device_state(dev)["coef"]
    flags = diff._flags(True)
    voxels = DHW[0] * DHW[1] * DHW[2]
    pull_rows, step_rows = [], []
    for N in (1, 8):
        shape = (N, 1) + DHW
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(shape, device=dev, generator=gen)
        z = torch.randn(shape, device=dev, generator=gen)
        y = torch.rand(shape, device=dev, generator=gen)
        mo = torch.randn((N, 2) + DHW, device=dev, generator=gen)
        mo[:, 1].clamp_(-1, 1)
        sample, x0, xs = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        t = torch.full((N,), 5, dtype=torch.int64, device=dev)

        def plain_step():
            H.check(lib.ddpm3d_p_sample_step(H.ptr(mo), H.ptr(x), H.ptr(z), H.ptr(coef), H.ptr(t), N, voxels, flags,
                                             H.ptr(sample), H.ptr(x0), H.stream()))

        for name, fwhm in PULLS:
            pull = guidance.LowPassPull(fwhm, (2.0, 2.0, 2.0), measurement=y)
            passes = sum(r > 0 for r in pull.radii)

            def pull_only():
                pull.apply(mo, x, t, flags, diff, out=xs)

            def guided_step():
                pull.apply(mo, x, t, flags, diff, out=xs)
                H.check(lib.ddpm3d_p_sample_step_x0(H.ptr(mo), H.ptr(xs), H.ptr(x), H.ptr(z), None, H.ptr(coef),
                                                    H.ptr(t), N, voxels, flags, H.ptr(sample), H.ptr(x0), H.stream()))

            ms = alternated({"pull": pull_only, "guided": guided_step, "plain": plain_step}, args.reps, args.inner)
            nbytes = (16.0 + 8.0 * max(passes - 1, 0)) * N * voxels
            row = dict(shape="%dx%dx%dx%d" % ((N,) + DHW), pull=name, radii=list(pull.radii), passes=passes,
                       nominal_mb=nbytes * 1e-6, **summary(ms["pull"]))
            row["gb_per_s"] = nbytes / row["ms"] * 1e-6
            pull_rows.append(row)
            step_rows.append(dict(shape=row["shape"], pull=name, guided=summary(ms["guided"]),
                                  unguided=summary(ms["plain"])))
            print("pull  %-12s %-26s %8.4f ms (%7.1f GB/s nominal); pull + step_x0 %8.4f ms, un-guided step %8.4f ms"
                  % (row["shape"], name, row["ms"], row["gb_per_s"], step_rows[-1]["guided"]["ms"],
                     step_rows[-1]["unguided"]["ms"]), flush=True)
        del x, z, y, mo, sample, x0, xs
        torch.cuda.empty_cache()
    return pull_rows, step_rows


def loop_rows(args, dev):
    model, diff, _ = bench.build_model(bench.PUBLISHED, args.respacing, dev)
    T = diff.num_timesteps
    shape = (1, 1) + DHW
    kw = {"low_res": torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)}
    rows = []
    for name, fwhm in PULLS:
        pull = guidance.LowPassPull(fwhm, (2.0, 2.0, 2.0))
        ms = host_timed({"unguided": lambda: diff.p_sample_loop(model, shape, model_kwargs=kw),
                         "guided": lambda: diff.p_sample_loop(model, shape, model_kwargs=kw, guide=pull)},
                        args.reps, T)
        row = dict(loop="p_sample_loop", shape=list(shape), steps=T, reps=args.reps, pull=name,
                   unguided=summary(ms["unguided"]), guided=summary(ms["guided"]))
        row["difference_ms_per_step"] = row["guided"]["ms"] - row["unguided"]["ms"]
        rows.append(row)
        print("loop  p_sample_loop 1x96^3, %s: %.3f ms/step un-guided (scatter %.3f), %.3f guided (scatter %.3f)"
              % (name, row["unguided"]["ms"], row["unguided"]["scatter_ms"], row["guided"]["ms"],
                 row["guided"]["scatter_ms"]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--respacing", default="10")
    ap.add_argument("--no-loops", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guidance_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps}
    res["pull"], res["step"] = kernel_rows(args, dev)
    if not args.no_loops:
        res["loops"] = loop_rows(args, dev)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
