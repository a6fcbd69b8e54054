#!/usr/bin/env python3
"""
Device-event times of the multi-scale SSIM entries beside ddpm3d_ssim3d, back to back in one run:
ddpm3d_pool2 of one volume (ms and GB/s of nominal traffic: the input read once, the pooled volume written),
ddpm3d_msssim3d at M = 4 (130x200x200 and 700x440x440) and M = 5 (700x440x440 only: the small volume allows 4), and
ddpm3d_ssim3d of the same pair, one estimate against one target, each with and without a mask, with the ratio of each
multi-scale time to that run's ddpm3d_ssim3d time (masked against masked).  The unmasked entry is timed at every
M from 1 up, so that the differences show what each further scale costs.

    python tools/msssim_time.py [--reps 10] [--json out.json]
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-denoising-diffusion-model_amd"))

import numpy as np
import torch

from guided_diffusion import _hip as H

SHAPES = [((130, 200, 200), (4,)), ((700, 440, 440), (4, 5))]


def timed(fn, reps):
    """median, min and max device time of fn() in ms over reps runs, after two warm-up runs"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    lib = H.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for shape, all_scales in SHAPES:
        D, Hh, W = shape
        voxels = D * Hh * W
        pooled = (D // 2) * (Hh // 2) * (W // 2)
        name = "%dx%dx%d" % shape
        y = torch.rand(shape, device=dev, generator=gen)
        x = y + 0.05 * torch.randn(shape, device=dev, generator=gen)
        mask = (y > 0.5).to(torch.uint8)
        half = torch.empty((D // 2, Hh // 2, W // 2), dtype=torch.float32, device=dev)
        half_mask = torch.empty((D // 2, Hh // 2, W // 2), dtype=torch.uint8, device=dev)
        need = max([lib.ddpm3d_ssim3d_workspace_bytes(1, D, Hh, W)]
                   + [lib.ddpm3d_msssim3d_workspace_bytes(1, D, Hh, W, M) for M in all_scales])
        ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        out = torch.empty((1, H.MSSSIM_MAX_SCALES, 3), dtype=torch.float64, device=dev)

        def pool(m=None, mo=None):
            H.check(lib.ddpm3d_pool2(H.ptr(x), H.ptr(m), 1, D, Hh, W, H.ptr(half), H.ptr(mo), H.stream()))

        def ssim(m=None):
            H.check(lib.ddpm3d_ssim3d(H.ptr(x), H.ptr(y), H.ptr(m), 1, D, Hh, W, 1e-4, 9e-4, H.ptr(ws), ws.numel() * 8,
                                      None, H.ptr(out), H.stream()))

        def msssim(M, m=None):
            H.check(lib.ddpm3d_msssim3d(H.ptr(x), H.ptr(y), H.ptr(m), 1, D, Hh, W, M, 1e-4, 9e-4, H.ptr(ws),
                                        ws.numel() * 8, H.ptr(out), H.stream()))

        cases = [("pool2", lambda: pool(), 4.0 * (voxels + pooled)),
                 ("pool2+mask", lambda: pool(mask, half_mask), 5.0 * (voxels + pooled)),
                 ("ssim3d", lambda: ssim(), 8.0 * voxels),
                 ("ssim3d+mask", lambda: ssim(mask), 9.0 * voxels)]
        for M in range(1, max(all_scales) + 1):         # every M: the differences are what each further scale costs
            cases.append(("msssim3d M=%d" % M, lambda M=M: msssim(M), None))
            if M in all_scales:
                cases.append(("msssim3d M=%d+mask" % M, lambda M=M: msssim(M, mask), None))
        base = {}
        for entry, fn, nbytes in cases:
            ms, lo, hi = timed(fn, args.reps)
            row = dict(entry=entry, shape=name, K=1, ms=ms, ms_min=lo, ms_max=hi)
            if nbytes is not None:
                row.update(gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6)
            if entry.startswith("ssim3d"):
                base[entry.endswith("+mask")] = ms
            if entry.startswith("msssim3d"):
                row["ratio_to_ssim3d"] = ms / base[entry.endswith("+mask")]     # masked against masked
            rows.append(row)
            print("%-22s %-12s %9.3f ms%s%s" % (entry, name, ms,
                                                "  %8.1f GB/s of %8.1f MB nominal" % (row["gb_per_s"], row["nominal_mb"])
                                                if nbytes is not None else "",
                                                "  %.3f x ssim3d" % row["ratio_to_ssim3d"]
                                                if "ratio_to_ssim3d" in row else ""), flush=True)
        del x, y, mask, half, half_mask, ws
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
