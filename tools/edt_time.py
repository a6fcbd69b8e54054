#!/usr/bin/env python3
"""
Device-event times of ddpm3d_distance_sq at 130x200x200 and 700x440x440 voxels of (3.27, 2, 2) mm on
three masks: lesions (balls, about 1 % foreground), a body (an ellipsoid, about 40 %) and all foreground, the worst
case of the scan.  The entry is three launches; its passes are timed by difference, on the same rows and the same
launch geometry: the D * H rows as D * H volumes of 1 x 1 x W run pass W alone, the D slices as D volumes of
1 x H x W run passes W and H, so pass H = the second - the first and pass D = the whole - the second.  Beside them, on
the same device: ddpm3d_label_components on the same mask (metrics.label_components, with its ranking and its copy),
and the streaming time of the three passes' nominal traffic, 21 bytes per voxel (torch copies: uint8 -> fp32, and
fp32 -> fp32 twice).  The entries of one case are timed in alternation: --rounds rounds, in each one window of
back-to-back calls per entry lasting at least --window seconds; reported are the median, the minimum and the maximum
over the rounds, GB/s of nominal traffic and the ratio to the streaming time.  metrics.boundary_target,
metrics.boundary (the target's side handed in) and metrics.edge_profile (three volumes) are timed as wholes on the
lesion mask against itself shifted by a voxel.  On this box's CPU, once per shape, on the body mask:
scipy.ndimage.distance_transform_edt (reported as absent where scipy is).

    python tools/edt_time.py [--window 0.2] [--rounds 5] [--no-cpu] [--json profiles/edt_time.json]
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

SHAPES = [(130, 200, 200), (700, 440, 440)]
SPACING = (3.27, 2.0, 2.0)
BYTES = {"pass W": 5, "pass H": 8, "pass D": 8, "distance_sq": 21}     # nominal, per voxel


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


def masks(shape, dev):
    """{name: uint8 (D, H, W)} on the device, from coordinates in [-1, 1]"""
    z, y, x = torch.meshgrid(*(torch.linspace(-1.0, 1.0, n, device=dev) for n in shape), indexing="ij")
    body = (z / 1.0) ** 2 + (y / 0.95) ** 2 + (x / 0.8) ** 2 <= 1.0
    rng = np.random.default_rng(7)
    lesions = torch.zeros(shape, dtype=torch.bool, device=dev)
    for _ in range(30):
        c = rng.uniform(-0.6, 0.6, size=3)
        lesions |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 0.086 ** 2
    return {"lesions": lesions.to(torch.uint8), "body": body.to(torch.uint8),
            "all foreground": torch.ones(shape, dtype=torch.uint8, device=dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edt_time: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    def med(v):
        return float(np.median(v))

    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        D, Hh, W = shape
        V = D * Hh * W
        all_masks = masks(shape, dev)
        for mask_name, mask in all_masks.items():
            share = float(mask.float().mean())
            vol = mask.float()
            dst, src = torch.empty_like(vol), torch.rand_like(vol)
            rows_w, slices = mask.view(D * Hh, 1, 1, W), mask.view(D, 1, Hh, W)

            def stream():
                dst.copy_(mask)
                dst.copy_(src)
                dst.copy_(src)

            entries = {"distance_sq": lambda: metrics.distance_sq(mask, SPACING),
                       "passes W + H": lambda: metrics.distance_sq(slices, SPACING),
                       "pass W": lambda: metrics.distance_sq(rows_w, SPACING),
                       "label_components": lambda: metrics.label_components(vol, 0.5),
                       "stream (21 B/voxel)": stream}
            try:
                metrics.label_components(vol, 0.5)
            except RuntimeError as e:                       # its device loops are capped: reported, not timed
                row(entry="label_components", shape=name, mask=mask_name, absent=True, reason=str(e))
                entries["label_components"] = lambda: None
            per, reps = alternate(entries, args.window, args.rounds)
            per["pass H"] = [a - b for a, b in zip(per["passes W + H"], per["pass W"])]
            per["pass D"] = [a - b for a, b in zip(per["distance_sq"], per["passes W + H"])]
            for entry in ("distance_sq", "pass W", "pass H", "pass D", "label_components", "stream (21 B/voxel)"):
                ms = per[entry]
                r = dict(entry=entry, shape=name, mask=mask_name, foreground=share, ms=med(ms), ms_min=min(ms),
                         ms_max=max(ms), rounds=len(ms))
                if entry in reps:
                    r["calls_per_window"] = reps[entry]
                else:
                    r["by_difference"] = True
                if entry in BYTES:
                    r["gb_per_s"] = BYTES[entry] * V / med(ms) * 1e-6
                if entry == "distance_sq":
                    r["times_stream"] = med([a / b for a, b in zip(ms, per["stream (21 B/voxel)"])])
                    r["times_label_components"] = med([a / b for a, b in zip(ms, per["label_components"])])
                row(**r)
            del entries, vol, dst, src
            torch.cuda.empty_cache()

        # the two consumers as wholes: the lesions against themselves shifted by a voxel along H
        lesions = all_masks["lesions"]
        labels, n = metrics.segment(lesions.float(), 0.5)
        estimate = torch.roll(labels, 1, dims=1).contiguous()
        volumes = {k: torch.rand(shape, device=dev) for k in ("target", "input", "denoised")}
        for entry, fn in (("boundary_target", lambda: metrics.boundary_target(labels, SPACING)),
                          ("boundary (target handed in)", None),
                          ("edge_profile (3 volumes, 3 + 5 shells of 2.5 mm)",
                           lambda: metrics.edge_profile(volumes, labels, SPACING, 2.5))):
            if fn is None:
                index = metrics.boundary_target(labels, SPACING)
                fn = lambda: metrics.boundary(labels, estimate, SPACING, index=index)
            per, reps = alternate({entry: fn}, args.window, args.rounds)
            row(entry=entry, shape=name, mask="lesions", regions=n, ms=med(per[entry]), ms_min=min(per[entry]),
                ms_max=max(per[entry]), rounds=len(per[entry]), calls_per_window=reps[entry])
        del volumes, labels, estimate, index
        torch.cuda.empty_cache()

        if not args.no_cpu:
            try:
                from scipy import ndimage
            except ImportError as e:
                row(entry="scipy.ndimage.distance_transform_edt (host, once)", shape=name, absent=True, reason=str(e))
            else:
                host = all_masks["body"].cpu().numpy()
                t0 = time.perf_counter()
                ndimage.distance_transform_edt(host, sampling=SPACING)
                row(entry="scipy.ndimage.distance_transform_edt (host, once)", shape=name, mask="body",
                    ms=(time.perf_counter() - t0) * 1e3)
                del host
        del all_masks
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
