#!/usr/bin/env python3
"""
Wall time per step of calc_bpd_loop against p_sample_loop on the published network, one process, one device:
both loops of the same schedule on the same 1 x 64^3 volume, alternated (--reps rounds of one loop each), host clock
around each whole loop ending in a device synchronise.  Per step, the bound runs one q_sample launch, the forward and
one VLB-terms launch with its fold; the sampler runs the forward and one update launch.  Prints one JSON line.

    python tools/bpd_time.py [--precision f16x3] [--respacing 250] [--reps 3] [--out bpd_time.json]
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
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--respacing", default="250")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bpd_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    model, diff, _ = bench.build_model(bench.PUBLISHED, a.respacing, dev)
    model.conv_precision = a.precision
    T = diff.num_timesteps
    shape = (1, 1, a.size, a.size, a.size)
    xs = torch.from_numpy(synth.synth_x_start(shape)).to(dev)
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)
    kw = {"low_res": lr}

    def bound():
        return diff.calc_bpd_loop(model, xs, model_kwargs=kw)["total_bpd"]

    def sample():
        return diff.p_sample_loop(model, shape, model_kwargs=kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / T

    for _ in range(a.warmup):
        timed(bound)
        timed(sample)
    ms = {"bound": [], "sample": []}
    for _ in range(a.reps):
        ms["bound"].append(timed(bound))
        ms["sample"].append(timed(sample))
    res = {
        "what": "calc_bpd_loop vs p_sample_loop, ms per step (host clock around a whole loop, device synchronised)",
        "network": "published (SuperResModel_noatt, 128 ch, mult (1,1,2,3,4))", "precision": a.precision,
        "shape": list(shape), "respacing": a.respacing, "steps": T, "reps": a.reps,
        "calc_bpd_loop_ms_per_step": min(ms["bound"]), "p_sample_loop_ms_per_step": min(ms["sample"]),
        "ratio_min": min(ms["bound"]) / min(ms["sample"]),
        "all_ms_per_step": ms, "device": torch.cuda.get_device_name(dev),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
