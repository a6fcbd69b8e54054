#!/usr/bin/env python3
"""
Device-event times of ddpm3d_project at 96^3, 130x200x200 and 700x440x440 with the default plan
(2 mm voxels, pitch = step = 2 mm, bins = samples = the slice's diagonal), both modes, for 1 and 36 angles and for 1
and 8 volumes.  Beside them, on the same device: one streaming read of the volumes (torch.sum), and, for one volume,
torch.nn.functional.grid_sample + amax over the same rays (bilinear, one call per angle; it pads with zeros where the
kernel does not count, so it is a time to compare, not a value).  On this box's CPU, once per shape and for one angle:
scipy.ndimage.rotate(order=1) + max (reported as absent where scipy is).  The entries of one (shape, angles, B) are
timed in alternation: --rounds rounds, in each one window of back-to-back calls per entry lasting at least --window
seconds; reported are the median, the minimum and the maximum over the rounds, the samples marched per second (every
sample of every ray, counted or not) and the ratio to the streaming read.  A case that does not fit the board's free
memory is skipped and listed as such.

    python tools/projection_time.py [--window 0.2] [--rounds 5] [--no-cpu] [--json profiles/projection_time.json]
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

from guided_diffusion import metrics

SHAPES = [(96, 96, 96), (130, 200, 200), (700, 440, 440)]
ANGLE_COUNTS = [1, 36]
BATCHES = [1, 8]
SPACING = (2.0, 2.0, 2.0)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(entries, seconds, rounds):
    """{name: [ms per call, one per round]}: every round times each entry once, in turn"""
    reps = {}
    for name, fn in entries.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(2, min(5000, int(seconds / max(time.perf_counter() - t0, 1e-6)) + 1))
    per = {name: [] for name in entries}
    for _ in range(rounds):
        for name, fn in entries.items():
            per[name].append(window(fn, reps[name]))
    return per, reps


def torch_mip(vol, plan):
    """the same rays through torch: per angle one grid_sample of the D slices and an amax over the samples"""
    D, Hh, W = plan.shape
    u = torch.arange(plan.bins, dtype=torch.float32, device=vol.device)[None, :]
    j = torch.arange(plan.samples, dtype=torch.float32, device=vol.device)[:, None]
    grids = []
    for h0, hu, hj, w0, wu, wj in plan.coef.tolist():
        x = (w0 + u * wu + j * wj) * (2.0 / (W - 1)) - 1.0
        y = (h0 + u * hu + j * hj) * (2.0 / (Hh - 1)) - 1.0
        grids.append(torch.stack([x, y], dim=-1)[None].expand(D, -1, -1, -1))
    src = vol[:, None]

    def run():
        return [torch.nn.functional.grid_sample(src, g, mode="bilinear", padding_mode="zeros",
                                                align_corners=True).amax(dim=2) for g in grids]

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("projection_time: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        V = shape[0] * shape[1] * shape[2]
        for A in ANGLE_COUNTS:
            plan = metrics.projection_plan(shape, SPACING, [k * 360.0 / A + (10.0 if A == 1 else 0.0) for k in range(A)])
            rays = A * shape[0] * plan.bins
            for B in BATCHES:
                free, _ = torch.cuda.mem_get_info(dev)
                need = 4 * (B * V + B * rays) + (4 * shape[0] * plan.bins * plan.samples * 3 if B == 1 else 0)
                if need > 0.8 * free:
                    row(entry="skipped", shape=name, angles=A, B=B,
                        reason="%.3g GB do not fit %.4g GB of free memory" % (need * 1e-9, free * 1e-9))
                    continue
                vol = torch.rand((B,) + shape, device=dev, generator=gen)
                entries = {"project max": lambda: metrics.project(vol, plan, mode="max"),
                           "project sum": lambda: metrics.project(vol, plan, mode="sum"),
                           "stream (torch.sum)": lambda: torch.sum(vol)}
                if B == 1:
                    entries["torch grid_sample + amax"] = torch_mip(vol[0], plan)
                per, reps = alternate(entries, args.window, args.rounds)
                stream = per["stream (torch.sum)"]
                for entry, ms in per.items():
                    med = float(np.median(ms))
                    r = dict(entry=entry, shape=name, angles=A, B=B, bins=plan.bins, samples=plan.samples, ms=med,
                             ms_min=min(ms), ms_max=max(ms), rounds=len(ms), calls_per_window=reps[entry])
                    if entry != "stream (torch.sum)":
                        r["gsamples_per_s"] = B * rays * plan.samples / med * 1e-6
                        r["times_stream"] = float(np.median([a / b for a, b in zip(ms, stream)]))
                    else:
                        r["gb_per_s"] = 4.0 * B * V / med * 1e-6
                    row(**r)
                if not args.no_cpu and B == 1 and A == 1:
                    try:
                        from scipy import ndimage
                    except ImportError as e:
                        row(entry="scipy.ndimage.rotate + max (host, once)", shape=name, absent=True, reason=str(e))
                    else:
                        host = vol[0].cpu().numpy()
                        t0 = time.perf_counter()
                        ndimage.rotate(host, 10.0, axes=(1, 2), reshape=True, order=1).max(axis=1)
                        row(entry="scipy.ndimage.rotate + max (host, once)", shape=name, angles=1, B=1,
                            ms=(time.perf_counter() - t0) * 1e3)
                        del host
                del vol, entries
                torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
