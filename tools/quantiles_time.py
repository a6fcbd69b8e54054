#!/usr/bin/env python3
"""
Device-event times of ddpm3d_draw_quantiles with three levels (0.025, 0.5, 0.975), without and with
a target, at K in {2, 8, 16, 64} draws of a 130x200x200 and a 700x440x440 volume, beside ddpm3d_draw_moments on the
same accumulators and weight sum in the same run and beside torch.sort along the draw axis on the same device; one
numpy.quantile of the small volume at K = 8 on this box's CPU, timed once, for scale.  The entries of one (shape, K) are
timed in alternation: --rounds rounds, in each one window of back-to-back calls per entry lasting at least --window
seconds; reported are the median, the minimum and the maximum over the rounds and the median of the per-round ratio
to draw_moments.  GB/s is of nominal traffic: K volumes (+ the weight sum, + the target) read once, the outputs
written once (3 quantile volumes, + 2 bytes per voxel of ranks with a target; mean and std for draw_moments).  A case
that does not fit the board's free memory is skipped and listed as such.

    python tools/quantiles_time.py [--window 0.2] [--rounds 5] [--no-cpu] [--json profiles/quantiles_time.json]
"""

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-denoising-diffusion-model_amd"))

import numpy as np
import torch

from guided_diffusion import _hip as H
from guided_diffusion import uncertainty

SHAPES = [(130, 200, 200), (700, 440, 440)]
DRAWS = [2, 8, 16, 64]
LEVELS = (0.025, 0.5, 0.975)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quantiles_time: needs a GPU; nothing is measured without one")
    lib = H.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    nq = len(LEVELS)
    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        n = int(np.prod(shape))
        free, total = torch.cuda.mem_get_info(dev)
        fits = [K for K in DRAWS if (K + 8) * n * 4 <= 0.9 * free]
        for K in DRAWS:
            if K not in fits:
                row(entry="skipped", shape=name, K=K, reason="K + 8 volumes of %.3g GB do not fit %.4g GB of free memory"
                    % (n * 4e-9, free * 1e-9))
        if not fits:
            continue
        acc_all = torch.empty((max(fits), n), dtype=torch.float32, device=dev)
        for k in range(max(fits)):                                   # unit noise on a level of 1, one volume at a time
            acc_all[k] = 1.0 + torch.randn(n, device=dev, generator=gen)
        wsum = 0.5 + torch.rand(n, device=dev, generator=gen)
        target = 1.0 + torch.randn(n, device=dev, generator=gen)
        quant = torch.empty((nq, n), dtype=torch.float32, device=dev)
        below = torch.empty(n, dtype=torch.uint8, device=dev)
        equal = torch.empty_like(below)
        mean = torch.empty(n, dtype=torch.float32, device=dev)
        std = torch.empty_like(mean)
        for K in fits:
            acc = acc_all[:K]
            lower, frac = uncertainty.quantile_positions(LEVELS, K)
            c_lower, c_frac = (ctypes.c_int * nq)(*lower), (ctypes.c_float * nq)(*frac)

            def quantiles():
                H.check(lib.ddpm3d_draw_quantiles(H.ptr(acc), H.ptr(wsum), K, n, nq, c_lower, c_frac, None, H.ptr(quant),
                                                  None, None, H.stream()))

            def quantiles_target():
                H.check(lib.ddpm3d_draw_quantiles(H.ptr(acc), H.ptr(wsum), K, n, nq, c_lower, c_frac, H.ptr(target),
                                                  H.ptr(quant), H.ptr(below), H.ptr(equal), H.stream()))

            def moments():
                H.check(lib.ddpm3d_draw_moments(H.ptr(acc), H.ptr(wsum), K, n, H.ptr(mean), H.ptr(std), H.stream()))

            entries = {"draw_quantiles": quantiles, "draw_quantiles + target": quantiles_target,
                       "draw_moments": moments}
            free, _ = torch.cuda.mem_get_info(dev)
            sort_fits = K * n * (4 + 8) * 1.1 <= free                # torch.sort returns values and int64 indices
            if sort_fits:
                entries["torch.sort(dim=0)"] = lambda: torch.sort(acc, dim=0)
            else:
                row(entry="skipped", shape=name, K=K, reason="torch.sort's values and indices (%.4g GB) do not fit %.4g "
                    "GB of free memory" % (K * n * 12e-9, free * 1e-9))
            per, reps = alternate(entries, args.window, args.rounds)
            nbytes = {"draw_quantiles": 4.0 * n * (K + 1 + nq),
                      "draw_quantiles + target": 4.0 * n * (K + 2 + nq) + 2.0 * n,
                      "draw_moments": 4.0 * n * (K + 1 + 2), "torch.sort(dim=0)": 4.0 * n * 2 * K + 8.0 * n * K}
            for entry, ms in per.items():
                med = float(np.median(ms))
                ratio = float(np.median([a / b for a, b in zip(ms, per["draw_moments"])]))
                row(entry=entry, shape=name, K=K, levels=nq, ms=med, ms_min=min(ms), ms_max=max(ms), rounds=len(ms),
                    calls_per_window=reps[entry], nominal_mb=nbytes[entry] * 1e-6, gb_per_s=nbytes[entry] / med * 1e-6,
                    times_draw_moments=ratio)
            torch.cuda.empty_cache()
            if not args.no_cpu and shape == SHAPES[0] and K == 8:
                host = (acc / wsum).cpu().numpy()
                t0 = time.perf_counter()
                np.quantile(host, LEVELS, axis=0, method="linear")
                row(entry="numpy.quantile (host, fp32 in)", shape=name, K=K, levels=nq,
                    ms=(time.perf_counter() - t0) * 1e3, host_threads=torch.get_num_threads())
                del host
        del acc_all, wsum, target, quant, below, equal, mean, std
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
