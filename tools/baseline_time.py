#!/usr/bin/env python3
"""
Device-event times of the two baseline denoisers at 130x200x200 and 700x440x440: ddpm3d_gauss_smooth
at 4 mm and 8 mm FWHM on isotropic 2 mm voxels (radii 3 and 5), and ddpm3d_nlm at search 3 / patch 1 and search 5 /
patch 1 (h = 2 noise stds), beside one scipy.ndimage.gaussian_filter of the 4 mm case on this box's CPU, timed once,
for scale.  Each device figure is the median of three timed windows of at least --window seconds of back-to-back
calls, after a warm-up.  GB/s is of nominal traffic: for the Gaussian 8 bytes per voxel and pass (three passes), for
NLM the volume read once and written once; streaming_ms is that traffic at --hbm_tb_s, the rate this project's plain
streaming kernels reach on the chip.  For NLM gflop_per_s is of the naive operation count: per voxel and candidate 3
operations per patch tap (difference, square, add) and 4 for the weight and the two sums, every candidate of the box
counted.

    python tools/baseline_time.py [--window 0.3] [--no-cpu] [--json profiles/baseline_time.json]
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
from guided_diffusion import metrics

SHAPES = [(130, 200, 200), (700, 440, 440)]
SPACING = (2.0, 2.0, 2.0)
FWHMS = [4.0, 8.0]
WINDOWS = [(3, 1), (5, 1)]                                    # (search, patch) radii, the same on every axis


def windows(fn, seconds):
    """median, min and max ms per call over three windows of back-to-back calls lasting at least `seconds` each"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(2, min(5000, int(seconds / max(time.perf_counter() - t0, 1e-6)) + 1))
    per = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / reps)
    return float(np.median(per)), min(per), max(per), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--hbm_tb_s", type=float, default=5.3)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("baseline_time: needs a GPU; nothing is measured without one")
    lib = H.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        D, Hh, W = shape
        voxels = D * Hh * W
        x = 1.0 + torch.randn(shape, device=dev, generator=gen)           # unit noise on a level of 1
        out = torch.empty_like(x)
        ws = torch.empty(lib.ddpm3d_gauss_smooth_workspace_bytes(D, Hh, W) // 4, dtype=torch.float32, device=dev)
        for fwhm in FWHMS:
            t = metrics.gaussian_taps(fwhm, SPACING)

            def call():
                H.check(lib.ddpm3d_gauss_smooth(H.ptr(x), D, Hh, W, t.radii[0], t.radii[1], t.radii[2], t.tables[0],
                                                t.tables[1], t.tables[2], H.ptr(out), H.ptr(ws), ws.numel() * 4,
                                                H.stream()))

            ms, lo, hi, reps = windows(call, args.window)
            nbytes = 24.0 * voxels
            row(entry="gauss_smooth", shape=name, fwhm_mm=fwhm, radius=t.radii[0], ms=ms, ms_min=lo, ms_max=hi,
                calls_per_window=reps, gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6,
                streaming_ms=nbytes / (args.hbm_tb_s * 1e9), times_streaming=ms / (nbytes / (args.hbm_tb_s * 1e9)))
        if not args.no_cpu:
            from scipy import ndimage
            host = x.cpu().numpy()
            t0 = time.perf_counter()
            ndimage.gaussian_filter(host, metrics.gaussian_taps(FWHMS[0], SPACING).sigma_voxels, truncate=3.0)
            row(entry="scipy.ndimage.gaussian_filter (host, fp32)", shape=name, fwhm_mm=FWHMS[0],
                ms=(time.perf_counter() - t0) * 1e3, host_threads=torch.get_num_threads())
            del host
        for search, patch in WINDOWS:

            def call():
                H.check(lib.ddpm3d_nlm(H.ptr(x), D, Hh, W, search, search, search, patch, patch, patch, 2.0, 0.0,
                                       H.ptr(out), H.stream()))

            ms, lo, hi, reps = windows(call, args.window)
            nbytes = 8.0 * voxels
            n_s, n_p = (2 * search + 1) ** 3, (2 * patch + 1) ** 3
            flops = float(voxels) * n_s * (3 * n_p + 4)
            row(entry="nlm", shape=name, search=search, patch=patch, candidates=n_s, patch_taps=n_p, ms=ms, ms_min=lo,
                ms_max=hi, calls_per_window=reps, gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6,
                streaming_ms=nbytes / (args.hbm_tb_s * 1e9), times_streaming=ms / (nbytes / (args.hbm_tb_s * 1e9)),
                naive_gflop=flops * 1e-9, gflop_per_s=flops / ms * 1e-6)
        del x, out, ws
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
