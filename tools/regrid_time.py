#!/usr/bin/env python3
"""
Device-event times of ddpm3d_regrid at 130x200x200 and 700x440x440, linear and cubic: 2x up on every
axis, 2x down on every axis, and an anisotropic scanner grid of 3.27 x 2.5 x 2.5 mm brought to 2 mm.  Each case is
timed as the one call regrid.apply makes and pass by pass (each pass as a call of its own on the extents its
predecessors leave), beside torch.nn.functional.interpolate(mode="trilinear") on the device for the growing linear
case and one scipy.ndimage.zoom(order=1) of the small 2x-up case on this box's CPU, timed once, for scale.  Each device
figure is the median of three timed windows of at least --window seconds of back-to-back calls, after a warm-up.
GB/s is of nominal traffic: per pass its input read once and its output written once; streaming_ms is that traffic at
--hbm_tb_s, the rate this project's plain streaming kernels reach on the chip.

    python tools/regrid_time.py [--window 0.3] [--no-cpu] [--json profiles/regrid_time.json]
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
from guided_diffusion import regrid

SHAPES = [(130, 200, 200), (700, 440, 440)]
CASES = {
    "up2": lambda s: tuple(2 * v for v in s),
    "down2": lambda s: tuple(v // 2 for v in s),
    "aniso_3.27x2.5x2.5_to_2mm": lambda s: regrid.grid_shape(s, (3.27, 2.5, 2.5), (2.0, 2.0, 2.0)),
}


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


def passes_of(shape_in, shape_out):
    """[(axis name, extents before, extents after)] of the passes ddpm3d_regrid launches, in its order W, H, D"""
    cur, out = list(shape_in), []
    for axis in (2, 1, 0):
        if shape_in[axis] != shape_out[axis]:
            nxt = list(cur)
            nxt[axis] = shape_out[axis]
            out.append(("DHW"[axis], tuple(cur), tuple(nxt)))
            cur = nxt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--hbm_tb_s", type=float, default=5.3)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("regrid_time: needs a GPU; nothing is measured without one")
    lib = H.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    def timed(plan, x):
        """ms of one ddpm3d_regrid call of this plan on x, buffers allocated once"""
        need = lib.ddpm3d_regrid_workspace_bytes(1, *plan.shape_in, *plan.shape_out)
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        out = torch.empty(plan.shape_out, dtype=torch.float32, device=dev)
        axes, _ = plan.device_axes(dev)

        def call():
            H.check(lib.ddpm3d_regrid(H.ptr(x), 1, *plan.shape_in, axes, H.ptr(out), H.ptr(ws), need, H.stream()))

        return windows(call, args.window)

    def streaming(nbytes):
        return nbytes / (args.hbm_tb_s * 1e9)

    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        x = 1.0 + torch.randn(shape, device=dev, generator=gen)           # unit noise on a level of 1
        for case, to in CASES.items():
            shape_out = to(shape)
            steps = passes_of(shape, shape_out)
            for mode in ("linear", "cubic"):
                plan = regrid.plan(shape, shape_out, mode)
                nbytes = 4.0 * sum(int(np.prod(a)) + int(np.prod(b)) for _, a, b in steps)
                ms, lo, hi, reps = timed(plan, x)
                row(entry="regrid", shape=name, case=case, mode=mode, shape_out="%dx%dx%d" % shape_out,
                    passes="".join(p[0] for p in steps), taps=[a.taps for a in plan.axes], ms=ms, ms_min=lo, ms_max=hi,
                    calls_per_window=reps, gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6,
                    streaming_ms=streaming(nbytes), times_streaming=ms / streaming(nbytes))
                for axis, before, after in steps:
                    y = 1.0 + torch.randn(before, device=dev, generator=gen)
                    one = regrid.plan(before, after, mode)
                    nb = 4.0 * (int(np.prod(before)) + int(np.prod(after)))
                    ms, lo, hi, reps = timed(one, y)
                    row(entry="regrid pass", shape=name, case=case, mode=mode, axis=axis,
                        before="%dx%dx%d" % before, after="%dx%dx%d" % after, taps=max(a.taps for a in one.axes), ms=ms,
                        ms_min=lo, ms_max=hi, calls_per_window=reps, gb_per_s=nb / ms * 1e-6, nominal_mb=nb * 1e-6,
                        streaming_ms=streaming(nb), times_streaming=ms / streaming(nb))
                    del y
                    torch.cuda.empty_cache()
            if case == "up2":
                x5 = x[None, None]

                def call():
                    torch.nn.functional.interpolate(x5, size=shape_out, mode="trilinear", align_corners=False)

                ms, lo, hi, reps = windows(call, args.window)
                nb = 4.0 * (int(np.prod(shape)) + int(np.prod(shape_out)))       # one pass: read once, write once
                row(entry="torch interpolate(trilinear) (device)", shape=name, case=case, ms=ms, ms_min=lo, ms_max=hi,
                    calls_per_window=reps, gb_per_s=nb / ms * 1e-6, nominal_mb=nb * 1e-6)
                torch.cuda.empty_cache()
                if not args.no_cpu and shape == SHAPES[0]:
                    from scipy import ndimage
                    host = x.cpu().numpy()
                    t0 = time.perf_counter()
                    ndimage.zoom(host, 2.0, order=1, grid_mode=True, mode="nearest")
                    row(entry="scipy.ndimage.zoom(order=1) (host, fp32)", shape=name, case=case,
                        ms=(time.perf_counter() - t0) * 1e3, host_threads=torch.get_num_threads())
                    del host
        del x
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
