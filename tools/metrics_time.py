#!/usr/bin/env python3
"""
Device-event times of the two image-quality entries: ddpm3d_error_moments and ddpm3d_ssim3d at
130x200x200 and 700x440x440, K = 1 and 8 estimates against one target, SSIM with and without the map, as ms and
GB/s of nominal traffic (every input read once + the map written), beside the scipy fp64 time of the same SSIM on
this box's CPU (130x200x200 only).

    python tools/metrics_time.py [--reps 10] [--no-cpu] [--json out.json]
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-denoising-diffusion-model_amd"))

import numpy as np
import torch

from guided_diffusion import _hip as H

SHAPES = [(130, 200, 200), (700, 440, 440)]
KS = [1, 8]


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


def scipy_ssim_seconds(x, y):
    import scipy.ndimage
    x, y = x.astype(np.float64), y.astype(np.float64)
    t0 = time.perf_counter()
    f = lambda a: scipy.ndimage.gaussian_filter(a, 1.5, truncate=3.5)[5:-5, 5:-5, 5:-5]
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    s.mean()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    lib = H.load()
    dev = torch.device("cuda:0")
    rows = []
    gen = torch.Generator(device=dev).manual_seed(1)
    for shape in SHAPES:
        D, Hh, W = shape
        voxels = D * Hh * W
        interior = (D - 10) * (Hh - 10) * (W - 10)
        y = torch.rand(shape, device=dev, generator=gen)
        mask = (y > 0.5).to(torch.uint8)
        std = torch.rand(shape, device=dev, generator=gen) * 0.1
        for K in KS:
            x = y[None] + 0.05 * torch.randn((K,) + shape, device=dev, generator=gen)
            out = torch.empty((K, H.EM_REC), dtype=torch.float64, device=dev)
            ws = torch.empty(max(lib.ddpm3d_error_moments_workspace_bytes(K, voxels),
                                 lib.ddpm3d_ssim3d_workspace_bytes(K, D, Hh, W)) // 8, dtype=torch.float64, device=dev)
            smap = torch.empty((K, D - 10, Hh - 10, W - 10), dtype=torch.float32, device=dev)

            def moments(m=None, s=None):
                H.check(lib.ddpm3d_error_moments(H.ptr(x), H.ptr(y), H.ptr(m), H.ptr(s), K, voxels, H.ptr(ws),
                                                 ws.numel() * 8, H.ptr(out), H.stream()))

            def ssim(mp=None):
                H.check(lib.ddpm3d_ssim3d(H.ptr(x), H.ptr(y), None, K, D, Hh, W, 1e-4, 9e-4, H.ptr(ws),
                                          ws.numel() * 8, H.ptr(mp), H.ptr(out), H.stream()))

            cases = [
                ("error_moments", lambda: moments(), 4.0 * voxels * (K + 1)),
                ("error_moments+mask+std", lambda: moments(mask, std), 4.0 * voxels * (K + 2) + voxels),
                ("ssim3d", lambda: ssim(), 4.0 * voxels * (K + 1)),
                ("ssim3d+map", lambda: ssim(smap), 4.0 * voxels * (K + 1) + 4.0 * interior * K),
            ]
            for name, fn, nbytes in cases:
                ms, lo, hi = timed(fn, args.reps)
                rows.append(dict(entry=name, shape="%dx%dx%d" % shape, K=K, ms=ms, ms_min=lo, ms_max=hi,
                                 gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6))
                print("%-24s %-12s K=%d  %9.3f ms  %8.1f GB/s of %9.1f MB nominal"
                      % (name, rows[-1]["shape"], K, ms, rows[-1]["gb_per_s"], rows[-1]["nominal_mb"]), flush=True)
            del x, smap, ws
        if shape == SHAPES[0] and not args.no_cpu:
            xc, yc = (y + 0.05 * torch.randn(shape, device=dev, generator=gen)).cpu().numpy(), y.cpu().numpy()
            secs = min(scipy_ssim_seconds(xc, yc) for _ in range(2))
            rows.append(dict(entry="scipy fp64 ssim (host)", shape="%dx%dx%d" % shape, K=1, ms=secs * 1e3))
            print("%-24s %-12s K=1  %9.3f ms  (%d host threads visible to torch)"
                  % ("scipy fp64 ssim (host)", rows[-1]["shape"], secs * 1e3, torch.get_num_threads()), flush=True)
        del y, mask, std
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
