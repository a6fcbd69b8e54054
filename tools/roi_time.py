#!/usr/bin/env python3
"""
Device-event times of the per-region statistics: building the region index (metrics.roi_index) and
ddpm3d_roi_moments (metrics.roi_moments' launch, against a target) at 130x200x200 and 700x440x440 with seeded
synthetic labels -- a body (an elliptic cylinder of about 40 % of the voxels), one organ-sized box and twenty spheres
of radius 3..10 voxels -- for K = 1 and 8 estimates, beside scipy.ndimage's labelled mean, standard deviation,
maximum and minimum of one estimate on this box's CPU.  Each figure is the median of three timed windows of at least
--window seconds of back-to-back calls, after a warm-up; GB/s is of nominal traffic (per estimate and entry: 8 bytes
of index, 4 of the estimate, 4 of the target).

    python tools/roi_time.py [--window 0.3] [--no-cpu] [--json profiles/roi_time.json]
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
KS = [1, 8]
BODY, ORGAN, FIRST_SPHERE, SPHERES = 1, 2, 3, 20


def synthetic_labels(shape, dev, seed=7):
    """(D, H, W) int32 on the device: body 1, organ 2, spheres 3..22 (later labels overwrite earlier ones)"""
    D, Hh, W = shape
    rng = np.random.default_rng(seed)
    h = torch.arange(Hh, device=dev, dtype=torch.float32)[:, None]
    w = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    inside = ((h - Hh / 2) / (0.36 * Hh)) ** 2 + ((w - W / 2) / (0.36 * W)) ** 2 <= 1.0      # pi * 0.36^2 = 0.407
    lab = inside.to(torch.int32)[None].repeat(D, 1, 1) * BODY
    lab[D // 4:D // 4 + D // 5, Hh // 3:Hh // 3 + Hh // 4, W // 3:W // 3 + W // 4] = ORGAN
    for i in range(SPHERES):
        r = int(rng.integers(3, 11))
        c = [int(rng.integers(r, n - r)) for n in shape]
        ax = [torch.arange(ci - r, ci + r + 1, device=dev) - ci for ci in c]
        ball = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2 <= r * r
        box = lab[c[0] - r:c[0] + r + 1, c[1] - r:c[1] + r + 1, c[2] - r:c[2] + r + 1]
        box[ball] = FIRST_SPHERE + i
    return lab


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


def scipy_seconds(x, lab, found):
    from scipy import ndimage
    t0 = time.perf_counter()
    for f in (ndimage.mean, ndimage.standard_deviation, ndimage.maximum, ndimage.minimum):
        f(x, lab, found)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("roi_time: needs a GPU; nothing is measured without one")
    lib = H.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        lab = synthetic_labels(shape, dev)
        index = metrics.roi_index(lab)
        entries = index.offsets[-1]
        share = {"body": index.counts[0] / index.voxels, "organ": index.counts[1] / index.voxels}
        ms, lo, hi, reps = windows(lambda: metrics.roi_index(lab), args.window)
        row(entry="roi_index", shape=name, regions=len(index), entries=entries, body_share=share["body"],
            organ_share=share["organ"], ms=ms, ms_min=lo, ms_max=hi, calls_per_window=reps)
        y = torch.rand(shape, device=dev, generator=gen)
        for K in KS:
            x = y[None] + 0.05 * torch.randn((K,) + shape, device=dev, generator=gen)
            ws = torch.empty(lib.ddpm3d_roi_moments_workspace_bytes(K, index.desc) // 8, dtype=torch.float64,
                             device=dev)
            out = torch.empty((K, len(index), H.ROI_REC), dtype=torch.float64, device=dev)

            def moments():
                H.check(lib.ddpm3d_roi_moments(H.ptr(x), H.ptr(y), K, index.voxels, index.desc, H.ptr(ws),
                                               ws.numel() * 8, H.ptr(out), H.stream()))

            ms, lo, hi, reps = windows(moments, args.window)
            nbytes = 16.0 * entries * K
            row(entry="roi_moments", shape=name, K=K, entries=entries, ms=ms, ms_min=lo, ms_max=hi,
                calls_per_window=reps, gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6)
            if K == 1 and not args.no_cpu:
                secs = scipy_seconds(x[0].cpu().numpy(), lab.cpu().numpy(), index.labels)
                row(entry="scipy.ndimage mean+std+max+min (host, one estimate)", shape=name, K=1, ms=secs * 1e3,
                    host_threads=torch.get_num_threads())
            del x, ws, out
        del y, lab, index
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
