#!/usr/bin/env python3
"""
Device-event times of the lesion segmentation: ddpm3d_label_components alone (the entry's four
launches), metrics.label_components (the entry plus the ranking of the roots with torch ops and its one
device-to-host copy) and metrics.segment (plus the size filter, min_voxels = 10) at 130x200x200 and 700x440x440, for
connectivity 6 and 26, on a seeded synthetic target -- an elliptic-cylinder body of about 40 % of the voxels with
forty hot spheres of radius 3..10 voxels inside it, plus Gaussian noise -- thresholded at the quantile that leaves
roughly 1 % and roughly 40 % of the voxels as foreground (estimated from a million sampled voxels), beside one
scipy.ndimage.label call on the host copy of the same mask on this box's CPU, whose component count must agree.
Each figure is the median of three timed windows of at least --window seconds of back-to-back calls, after a
warm-up; GB/s is of nominal traffic: 4 bytes of `vol` read and 4 bytes of `roots` written per voxel.

    python tools/segment_time.py [--window 0.3] [--no-cpu] [--json profiles/segment_time.json]
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
CONNECTIVITIES = [6, 26]
SHARES = [0.01, 0.40]
SPHERES = 40
MIN_VOXELS = 10


def synthetic_target(shape, dev, seed=7):
    """(D, H, W) float32 on the device: body 0.25, spheres of uptake 0.5..1, noise of sigma 0.05"""
    D, Hh, W = shape
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device=dev).manual_seed(seed)
    h = torch.arange(Hh, device=dev, dtype=torch.float32)[:, None]
    w = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    inside = ((h - Hh / 2) / (0.36 * Hh)) ** 2 + ((w - W / 2) / (0.36 * W)) ** 2 <= 1.0      # pi * 0.36^2 = 0.407
    vol = (inside.to(torch.float32) * 0.25)[None].repeat(D, 1, 1)
    for _ in range(SPHERES):
        r = int(rng.integers(3, 11))
        c = [int(rng.integers(n // 4, n - n // 4)) for n in shape]
        ax = [torch.arange(ci - r, ci + r + 1, device=dev) - ci for ci in c]
        ball = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2 <= r * r
        box = vol[c[0] - r:c[0] + r + 1, c[1] - r:c[1] + r + 1, c[2] - r:c[2] + r + 1]
        box[ball] = float(rng.uniform(0.5, 1.0))
    vol += 0.05 * torch.randn(shape, device=dev, generator=gen)
    return vol.contiguous()


def threshold_for(vol, share, seed=3):
    """the value that roughly `share` of the voxels exceed, from a million sampled voxels"""
    gen = torch.Generator(device=vol.device).manual_seed(seed)
    at = torch.randint(0, vol.numel(), (1 << 20,), device=vol.device, generator=gen)
    return float(torch.quantile(vol.reshape(-1)[at], 1.0 - share))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segment_time: needs a GPU; nothing is measured without one")
    lib = H.load()
    dev = torch.device("cuda:0")
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        vol = synthetic_target(shape, dev)
        D, Hh, W = shape
        need = lib.ddpm3d_label_components_workspace_bytes(D, Hh, W)
        ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
        roots = torch.empty(shape, dtype=torch.int32, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        nbytes = 8.0 * vol.numel()
        for share in SHARES:
            threshold = threshold_for(vol, share)
            foreground = float((vol > threshold).float().mean())
            host = None if args.no_cpu else (vol > threshold).cpu().numpy()
            for connectivity in CONNECTIVITIES:
                def entry():
                    H.check(lib.ddpm3d_label_components(H.ptr(vol), None, threshold, connectivity, D, Hh, W,
                                                        H.ptr(roots), H.ptr(ws), need, H.ptr(status), H.stream()))

                common = dict(shape=name, connectivity=connectivity, foreground=foreground)
                ms, lo, hi, reps = windows(entry, args.window)
                overrun, n = status.cpu().tolist()
                row(entry="ddpm3d_label_components", ms=ms, ms_min=lo, ms_max=hi, calls_per_window=reps,
                    gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6, components=n, overrun=overrun,
                    workspace_mb=need * 1e-6, **common)
                ms, lo, hi, reps = windows(lambda: metrics.label_components(vol, threshold, connectivity), args.window)
                row(entry="metrics.label_components", ms=ms, ms_min=lo, ms_max=hi, calls_per_window=reps, **common)
                kept = metrics.segment(vol, threshold, connectivity, MIN_VOXELS)[1]
                ms, lo, hi, reps = windows(lambda: metrics.segment(vol, threshold, connectivity, MIN_VOXELS),
                                           args.window)
                row(entry="metrics.segment", min_voxels=MIN_VOXELS, regions=kept, ms=ms, ms_min=lo, ms_max=hi,
                    calls_per_window=reps, **common)
                if host is not None:
                    from scipy import ndimage
                    t0 = time.perf_counter()
                    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
                    _, n_host = ndimage.label(host, structure=structure)
                    row(entry="scipy.ndimage.label (host, one core)", ms=(time.perf_counter() - t0) * 1e3,
                        components=int(n_host), agrees=bool(n_host == n), **common)
            del host
        del vol, ws, roots, status
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
