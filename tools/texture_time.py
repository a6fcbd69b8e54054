#!/usr/bin/env python3
"""
Device-event times of the per-region texture entry: ddpm3d_roi_texture at 130x200x200 and 700x440x440
over tools/roi_time.py's 22 synthetic regions and over one region holding 41 % of the voxels (the elliptic cylinder
alone: the whole-body single-region case, where every workgroup adds into one matrix), for 32 and 64 grey levels and
B = 1 and 8 estimates, alternated window by window with ddpm3d_roi_moments on the same index and buffers.  The
estimates are uniform noise (the matrix is dense: every cell is flushed) and, for the single region at B = 1, also a
smooth field plus a little noise (the matrix is a narrow band: the LDS atomics collide).  Each figure is the median of
three timed windows of at least --window seconds of back-to-back calls, after a warm-up; GB/s is of nominal traffic
(per estimate and entry: 8 bytes of index, 4 of the estimate, 2 of region_of, each read once).  The numpy restatement
of tests/texture_ref.py is timed once on the host at the small size, for scale.

    python tools/texture_time.py [--window 0.3] [--no-cpu] [--quick] [--label TEXT] [--json profiles/texture_time.json]

--quick keeps the single-region rows of the large size only (to compare builds of the library, selected with
DDPM3D_LIB); --label is copied into every row.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-denoising-diffusion-model_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from guided_diffusion import _hip as H
from guided_diffusion import metrics
from roi_time import SHAPES, synthetic_labels

LEVELS = [32, 64]
KS = [1, 8]


def alternated(fns, seconds):
    """per function the median, min and max ms per call over three windows of back-to-back calls lasting at least
    `seconds` each; the windows of the functions alternate"""
    reps = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps.append(max(3, min(5000, int(seconds / max(time.perf_counter() - t0, 1e-6)) + 1)))
    per = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps[i]):
                fn()
            b.record()
            b.synchronize()
            per[i].append(a.elapsed_time(b) / reps[i])
    return [(float(np.median(p)), min(p), max(p), n) for p, n in zip(per, reps)]


def smooth_field(shape, dev, gen):
    """a low-frequency field in about [0.1, 0.9] plus noise of sigma 0.01: neighbours share a grey level or differ by 1"""
    coarse = torch.rand((1, 1) + tuple(max(2, n // 40) for n in shape), device=dev, generator=gen)
    field = torch.nn.functional.interpolate(coarse, size=shape, mode="trilinear", align_corners=True)[0, 0]
    return (0.1 + 0.8 * field + 0.01 * torch.randn(shape, device=dev, generator=gen)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("texture_time: needs a GPU; nothing is measured without one")
    lib = H.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []

    def row(**kw):
        if args.label:
            kw["label"] = args.label
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    for shape in SHAPES[1:] if args.quick else SHAPES:
        name = "%dx%dx%d" % shape
        lab = synthetic_labels(shape, dev)
        sets = {"22 regions": lab}
        # the single region is the cylinder alone, as roi_time draws it before the organ and the spheres overwrite it
        D, Hh, W = shape
        h = torch.arange(Hh, device=dev, dtype=torch.float32)[:, None]
        w = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
        inside = ((h - Hh / 2) / (0.36 * Hh)) ** 2 + ((w - W / 2) / (0.36 * W)) ** 2 <= 1.0
        sets["one region"] = inside.to(torch.int32)[None].repeat(D, 1, 1).contiguous()
        y = torch.rand(shape, device=dev, generator=gen)
        for set_name, labels in sets.items():
            if args.quick and set_name != "one region":
                continue
            index = metrics.roi_index(labels)
            region_of = index.region_of()
            entries, R = index.offsets[-1], len(index)
            for K in KS[:1] if args.quick else KS:
                x = (y[None] + 0.05 * torch.randn((K,) + shape, device=dev, generator=gen)).contiguous()
                data = {"uniform": x}
                if set_name == "one region" and K == 1:
                    data["smooth"] = smooth_field(shape, dev, gen)[None].contiguous()
                ws = torch.empty(lib.ddpm3d_roi_moments_workspace_bytes(K, index.desc) // 8, dtype=torch.float64,
                                 device=dev)
                rec = torch.empty((K, R, H.ROI_REC), dtype=torch.float64, device=dev)
                for kind, est in data.items():
                    for levels in LEVELS:
                        lo = torch.zeros((K, R), device=dev)
                        inv_w = torch.full((K, R), float(levels), device=dev)          # bins of 1 / levels over [0, 1)
                        out = [torch.empty(K * R * n, dtype=torch.int64, device=dev)
                               for n in (levels * levels, levels, H.TEX_REC)]

                        def texture():
                            H.check(lib.ddpm3d_roi_texture(H.ptr(est), K, D, Hh, W, index.desc, H.ptr(region_of),
                                                           H.ptr(lo), H.ptr(inv_w), levels, H.ptr(out[0]),
                                                           H.ptr(out[1]), H.ptr(out[2]), H.stream()))

                        def moments():
                            H.check(lib.ddpm3d_roi_moments(H.ptr(est), 0, K, index.voxels, index.desc, H.ptr(ws),
                                                           ws.numel() * 8, H.ptr(rec), H.stream()))

                        (ms, lo_ms, hi_ms, reps), (m_ms, m_lo, m_hi, _) = alternated([texture, moments], args.window)
                        counts = out[2].view(K, R, H.TEX_REC).sum(dim=(0, 1)).tolist()
                        nbytes = 14.0 * entries * K
                        row(entry="roi_texture", shape=name, regions=set_name, data=kind, levels=levels, K=K,
                            entries=entries, ms=ms, ms_min=lo_ms, ms_max=hi_ms, calls_per_window=reps,
                            gb_per_s=nbytes / ms * 1e-6, nominal_mb=nbytes * 1e-6, pairs=int(counts[H.TEX_PAIRS]),
                            pairs_per_ns=counts[H.TEX_PAIRS] / ms * 1e-6,
                            cells_nonzero=int((out[0] != 0).sum()), roi_moments_ms=m_ms, roi_moments_ms_min=m_lo,
                            roi_moments_ms_max=m_hi, ratio_to_roi_moments=ms / m_ms)
                if (set_name == "one region" and K == 1 and shape == SHAPES[0] and not args.no_cpu
                        and not args.quick):
                    import texture_ref
                    xh, lh = x[0].cpu().numpy(), labels.cpu().numpy()
                    t0 = time.perf_counter()
                    texture_ref.roi_texture(xh, lh, 0.0, 64.0, 64)
                    row(entry="numpy restatement (host, one estimate, 64 levels)", shape=name, regions=set_name, K=1,
                        ms=(time.perf_counter() - t0) * 1e3, host_threads=torch.get_num_threads())
                del x, data, ws, rec
            del index, region_of
            torch.cuda.empty_cache()
        del y, lab, sets
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
