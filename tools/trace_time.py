#!/usr/bin/env python3
"""
What the per-step convergence trace costs, one process, one device.

Entry alone: device-event times of ddpm3d_trace_moments with all four inputs (est, prev, own targets, own weights:
16 bytes per voxel) at B = 1 and 8 x 96^3 and at one 700x440x440 canvas, as ms and GB/s, beside the same run's
ddpm3d_error_moments on the same est / target buffers (est + one shared target).  A call is short, so `--inner`
calls sit between a pair of events.

Whole loop: p_sample_loop of the published network at 1 x 96^3 with and without trace=, alternated, host clock around
each whole loop ending in a device synchronise, as ms per step.  The untraced loop of the same run is the yardstick:
its own run-to-run scatter (max - min over the reps) is reported next to the difference of the medians.

    python tools/trace_time.py [--reps 5] [--inner 20] [--respacing 50] [--precision f16x3] [--json profiles/trace_time.json]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from guided_diffusion import _hip as H  # noqa: E402
from guided_diffusion import metrics, synth  # noqa: E402

ENTRY_CASES = [(1, (96, 96, 96)), (8, (96, 96, 96)), (1, (700, 440, 440))]


def timed(fn, reps, inner):
    """median, min and max device time of one fn() in ms: reps event pairs around `inner` calls each, after two
    warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return float(np.median(times)), min(times), max(times)


def entry_rows(args, dev):
    lib = H.load()
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for B, shape in ENTRY_CASES:
        voxels = shape[0] * shape[1] * shape[2]
        y = torch.rand((B, voxels), device=dev, generator=gen)
        x = y + 0.05 * torch.randn((B, voxels), device=dev, generator=gen)
        prev = x + 0.01 * torch.randn((B, voxels), device=dev, generator=gen)
        w = torch.rand((B, voxels), device=dev, generator=gen)
        ws = torch.empty(max(lib.ddpm3d_trace_moments_workspace_bytes(B, voxels),
                             lib.ddpm3d_error_moments_workspace_bytes(B, voxels)) // 8, dtype=torch.float64, device=dev)
        out = torch.empty((B, max(H.TR_REC, H.EM_REC)), dtype=torch.float64, device=dev)

        def trace():
            H.check(lib.ddpm3d_trace_moments(H.ptr(x), H.ptr(prev), H.ptr(y), H.ptr(w), B, voxels, voxels, voxels,
                                             H.ptr(ws), ws.numel() * 8, H.ptr(out), H.stream()))

        def moments():
            H.check(lib.ddpm3d_error_moments(H.ptr(x), H.ptr(y), None, None, B, voxels, H.ptr(ws), ws.numel() * 8,
                                             H.ptr(out), H.stream()))

        inner = args.inner if voxels < 10 ** 7 else 2
        for name, fn, nbytes in (("trace_moments", trace, 16.0 * B * voxels),
                                 ("error_moments", moments, 4.0 * voxels * (B + 1))):
            ms, lo, hi = timed(fn, args.reps, inner)
            rows.append(dict(entry=name, shape="%dx%dx%d" % shape, B=B, ms=ms, ms_min=lo, ms_max=hi,
                             gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6))
            print("%-14s %-12s B=%d  %9.4f ms  %8.1f GB/s of %9.1f MB nominal"
                  % (name, rows[-1]["shape"], B, ms, rows[-1]["gb_per_s"], rows[-1]["nominal_mb"]), flush=True)
        del x, y, prev, w, ws
        torch.cuda.empty_cache()
    return rows


def loop_row(args, dev):
    model, diff, _ = bench.build_model(bench.PUBLISHED, args.respacing, dev)
    model.conv_precision = args.precision
    T = diff.num_timesteps
    shape = (1, 1, 96, 96, 96)
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)
    target = torch.from_numpy(synth.synth_x_start(shape)).to(dev)
    kw = {"low_res": lr}

    def plain():
        return diff.p_sample_loop(model, shape, model_kwargs=kw)

    def traced():
        tr = metrics.StepTrace(target=target)
        out = diff.p_sample_loop(model, shape, model_kwargs=kw, trace=tr)
        tr.records()
        return out

    def per_step(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / T

    per_step(plain)
    per_step(traced)
    ms = {"plain": [], "traced": []}
    for _ in range(args.reps):
        ms["plain"].append(per_step(plain))
        ms["traced"].append(per_step(traced))
    row = {
        "what": "p_sample_loop with and without trace=, ms per step (host clock around a whole loop, device "
                "synchronised; the traced loop includes records())",
        "network": "published (SuperResModel_noatt, 128 ch, mult (1,1,2,3,4))", "precision": args.precision,
        "shape": list(shape), "respacing": args.respacing, "steps": T, "reps": args.reps,
        "plain_ms_per_step": float(np.median(ms["plain"])), "traced_ms_per_step": float(np.median(ms["traced"])),
        "difference_ms_per_step": float(np.median(ms["traced"]) - np.median(ms["plain"])),
        "plain_scatter_ms_per_step": max(ms["plain"]) - min(ms["plain"]),
        "all_ms_per_step": ms,
    }
    print("p_sample_loop 1x96^3, %d steps: %.3f ms/step plain, %.3f traced, difference %+.3f, plain scatter %.3f"
          % (T, row["plain_ms_per_step"], row["traced_ms_per_step"], row["difference_ms_per_step"],
             row["plain_scatter_ms_per_step"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--respacing", default="50")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trace_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "entries": entry_rows(args, dev)}
    if not args.no_loop:
        res["loop"] = loop_row(args, dev)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
