#!/usr/bin/env python3
"""
Wall time per step of DDIM inversion (ddim_reverse_sample_loop) against the DDIM sampler (ddim_sample_loop, eta = 0)
on the published network, one process, one device: both loops of the same schedule on the same 1 x 64^3 volume,
alternated (--reps rounds of one loop each), host clock around each whole loop ending in a device synchronise, for
each arithmetic mode in --precisions.  Per step, inversion runs the forward and one reverse-step launch; the sampler
runs the forward, a randn_like draw and one update launch.  Prints one JSON line.

    python tools/inversion_time.py [--precisions f16x3,bf16] [--respacing ddim50] [--reps 3] [--out inv.json]
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
from guided_diffusion import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="f16x3,bf16")
    ap.add_argument("--respacing", default="ddim50")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inversion_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    model, diff, _ = bench.build_model(bench.PUBLISHED, a.respacing, dev)
    T = diff.num_timesteps
    shape = (1, 1, a.size, a.size, a.size)
    xs = torch.from_numpy(synth.synth_x_start(shape)).to(dev)
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)
    kw = {"low_res": lr}

    def invert():
        return diff.ddim_reverse_sample_loop(model, xs, model_kwargs=kw)

    def sample():
        return diff.ddim_sample_loop(model, shape, model_kwargs=kw, eta=0.0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / T

    res = {
        "what": "ddim_reverse_sample_loop vs ddim_sample_loop(eta=0), ms per step (host clock around a whole loop, "
                "device synchronised)",
        "network": "published (SuperResModel_noatt, 128 ch, mult (1,1,2,3,4))", "shape": list(shape),
        "respacing": a.respacing, "steps": T, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
        "precisions": {},
    }
    for prec in a.precisions.split(","):
        if prec == "bf16":
            model.convert_to_bf16()
        else:
            model.convert_to_fp32()
            model.conv_precision = prec
        for _ in range(a.warmup):
            timed(invert)
            timed(sample)
        ms = {"invert": [], "sample": []}
        for _ in range(a.reps):
            ms["invert"].append(timed(invert))
            ms["sample"].append(timed(sample))
        res["precisions"][prec] = {
            "ddim_reverse_sample_loop_ms_per_step": min(ms["invert"]),
            "ddim_sample_loop_ms_per_step": min(ms["sample"]),
            "ratio_min": min(ms["invert"]) / min(ms["sample"]),
            "all_ms_per_step": ms,
        }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
