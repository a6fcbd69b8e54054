#!/usr/bin/env python3
"""
Device-event times of the radial-spectrum entries at 96^3, 130x200x200 and 700x440x440, Hann window:
ddpm3d_dft3 per pass (ddpm3d_dft3_pass) and in whole at B = 1 and 8, ddpm3d_shell_spectrum with and without a target
at B = 1 and 8, beside torch.fft.rfftn on the same device (reported as absent if the call raises) and numpy.fft.rfftn
on this box's CPU, timed once.  The entries of one (shape, B) are timed in alternation: --rounds rounds, in each one
window of back-to-back calls per entry lasting at least --window seconds; reported are the median, the minimum and the
maximum over the rounds.  TFLOP/s is of the nominal count (2 V W for pass W, 8 D H Wh (H + D) for the other two, per
volume), GB/s of each pass's compulsory traffic (its input and output planes once).  A case that does not fit the
board's free memory is skipped and listed as such.

    python tools/spectrum_time.py [--window 0.2] [--rounds 5] [--no-cpu] [--json profiles/spectrum_time.json]
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

SHAPES = [(96, 96, 96), (130, 200, 200), (700, 440, 440)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spectrum_time: needs a GPU; nothing is measured without one")
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
        Wh = W // 2 + 1
        V, P = D * Hh * W, D * Hh * Wh
        plan = metrics.spectrum_plan(shape, SPACING)
        axes, index, _ = plan.on(dev)
        flops = {"pass W": 2.0 * V * W, "pass H": 8.0 * P * Hh, "pass D": 8.0 * P * D}
        flops["dft3"] = sum(flops.values())
        traffic = {"pass W": 4.0 * V + 8.0 * P, "pass H": 16.0 * P, "pass D": 16.0 * P}
        traffic["dft3"] = sum(traffic.values())
        for B in BATCHES:
            free, _ = torch.cuda.mem_get_info(dev)
            need = lib.ddpm3d_shell_spectrum_workspace_bytes(B, D, Hh, W, index.desc, 1)
            if (B + 1) * V * 4 + 3 * 8 * B * P + need > 0.9 * free:
                row(entry="skipped", shape=name, B=B, reason="%.3g GB do not fit %.4g GB of free memory"
                    % (((B + 1) * V * 4 + 24 * B * P + need) * 1e-9, free * 1e-9))
                continue
            vol = 1.0 + 0.1 * torch.randn((B,) + shape, device=dev, generator=gen)
            target = 1.0 + 0.1 * torch.randn(shape, device=dev, generator=gen)
            pivot = torch.ones(B, device=dev)
            out = torch.empty((2, B, P), dtype=torch.float32, device=dev)
            dft_ws = torch.empty(max(lib.ddpm3d_dft3_workspace_bytes(B, D, Hh, W), 16) // 4, dtype=torch.float32,
                                 device=dev)
            ws = torch.empty(max(need, 16) // 8, dtype=torch.float64, device=dev)
            rec = torch.empty((B, plan.shells, H.SP_REC), dtype=torch.float64, device=dev)

            def one_pass(which):
                return lambda: H.check(lib.ddpm3d_dft3_pass(which, H.ptr(vol), H.ptr(pivot), B, D, Hh, W, axes,
                                                            H.ptr(dft_ws), dft_ws.numel() * 4, H.ptr(out[0]),
                                                            H.ptr(out[1]), H.stream()))

            def dft3():
                H.check(lib.ddpm3d_dft3(H.ptr(vol), H.ptr(pivot), B, D, Hh, W, axes, H.ptr(dft_ws),
                                        dft_ws.numel() * 4, H.ptr(out[0]), H.ptr(out[1]), H.stream()))

            def spectrum(tgt):
                return lambda: H.check(lib.ddpm3d_shell_spectrum(
                    H.ptr(vol), H.ptr(pivot), H.ptr(tgt), H.ptr(pivot) if tgt is not None else None, B, D, Hh, W, axes,
                    index.desc, H.ptr(ws), ws.numel() * 8, H.ptr(rec), H.stream()))

            dft3()                                                       # the passes then read finite planes
            entries = {"pass W": one_pass(0), "pass H": one_pass(1), "pass D": one_pass(2), "dft3": dft3,
                       "shell_spectrum": spectrum(None), "shell_spectrum + target": spectrum(target)}
            try:
                torch.fft.rfftn(vol, dim=(1, 2, 3))
                torch.cuda.synchronize()
                entries["torch.fft.rfftn"] = lambda: torch.fft.rfftn(vol, dim=(1, 2, 3))
            except Exception as e:                                       # no FFT library behind torch on this box
                row(entry="torch.fft.rfftn", shape=name, B=B, absent=True, reason=str(e).splitlines()[0][:160])
            per, reps = alternate(entries, args.window, args.rounds)
            for entry, ms in per.items():
                med = float(np.median(ms))
                r = dict(entry=entry, shape=name, B=B, ms=med, ms_min=min(ms), ms_max=max(ms), rounds=len(ms),
                         calls_per_window=reps[entry])
                if entry != "torch.fft.rfftn":                           # a fast transform: the dense count is not its
                    key = entry if entry in flops else "dft3"
                    volumes = B + (1 if entry == "shell_spectrum + target" else 0)
                    r["nominal_tflop"] = flops[key] * volumes * 1e-12
                    r["tflop_per_s"] = flops[key] * volumes / med * 1e-9
                else:
                    r["times_dft3"] = float(np.median([a / b for a, b in zip(ms, per["dft3"])]))
                if entry in traffic:
                    r["compulsory_mb"] = traffic[entry] * B * 1e-6
                    r["gb_per_s"] = traffic[entry] * B / med * 1e-6
                row(**r)
            if not args.no_cpu and B == 1:
                host = vol[0].cpu().numpy()
                t0 = time.perf_counter()
                np.fft.rfftn(host)
                row(entry="numpy.fft.rfftn (host, once)", shape=name, B=1, ms=(time.perf_counter() - t0) * 1e3,
                    host_threads=torch.get_num_threads())
                del host
            del vol, target, out, dft_ws, ws, rec
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
