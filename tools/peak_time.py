#!/usr/bin/env python3
"""
Device-event times of the sphere-mean map behind SUVpeak: ddpm3d_sphere_mean at 130x200x200 and
700x440x440 for PERCIST's 1 cm^3 sphere on isotropic 2 mm voxels (123 taps) and 4 mm voxels (19 taps), B = 1 and 8
volumes per call, with and without a keep mask (90 % of the voxels at random), beside one scipy.ndimage.correlate of
the same footprint on this box's CPU, timed once, for scale.  Each device figure is the median of three timed windows
of at least --window seconds of back-to-back calls, after a warm-up; GB/s is of nominal traffic (vol read once plus
out written once: 8 bytes per voxel and volume), and streaming_ms is that traffic at --hbm_tb_s, the rate this
project's plain streaming kernels reach on the chip.

    python tools/peak_time.py [--window 0.3] [--no-cpu] [--json profiles/peak_time.json]
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
SPACINGS = [(2.0, 2.0, 2.0), (4.0, 4.0, 4.0)]
BS = [1, 8]


def windows(fn, seconds):
    """median, min and max ms per call over three windows of back-to-back calls lasting at least `seconds` each"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(3, min(5000, int(seconds / max(time.perf_counter() - t0, 1e-6)) + 1))
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


def scipy_seconds(x, fp):
    from scipy import ndimage
    r0, r1, r2 = fp.radii
    box = np.zeros((2 * r0 + 1, 2 * r1 + 1, 2 * r2 + 1), dtype=np.float32)
    for i, row in enumerate(fp.half_w):
        for j, w in enumerate(row):
            if w >= 0:
                box[i, j, r2 - w:r2 + w + 1] = 1.0 / fp.taps
    t0 = time.perf_counter()
    ndimage.correlate(x, box, mode="constant", cval=0.0)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--hbm_tb_s", type=float, default=5.3)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("peak_time: needs a GPU; nothing is measured without one")
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
        keep = (torch.rand(shape, device=dev, generator=gen) < 0.9).to(torch.uint8)
        for B in BS:
            x = torch.rand((B,) + shape, device=dev, generator=gen)
            out = torch.empty_like(x)
            for spacing in SPACINGS:
                fp = metrics.sphere_footprint(spacing)
                for k in (None, keep):

                    def call():
                        H.check(lib.ddpm3d_sphere_mean(H.ptr(x), H.ptr(k), B, D, Hh, W, fp.radii[0], fp.radii[1],
                                                       fp.table, H.ptr(out), H.stream()))

                    ms, lo, hi, reps = windows(call, args.window)
                    nbytes = 8.0 * voxels * B
                    row(entry="sphere_mean", shape=name, spacing_mm=spacing[0], taps=fp.taps, B=B, keep=k is not None,
                        ms=ms, ms_min=lo, ms_max=hi, calls_per_window=reps, gb_per_s=nbytes / ms * 1e-6,
                        nominal_mb=nbytes * 1e-6, streaming_ms=nbytes / (args.hbm_tb_s * 1e9),
                        times_streaming=ms / (nbytes / (args.hbm_tb_s * 1e9)))
                if B == 1 and not args.no_cpu:
                    secs = scipy_seconds(x[0].cpu().numpy(), fp)
                    row(entry="scipy.ndimage.correlate (host, one volume, fp32)", shape=name, spacing_mm=spacing[0],
                        taps=fp.taps, ms=secs * 1e3, host_threads=torch.get_num_threads())
            del x, out
            torch.cuda.empty_cache()
        del keep
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
