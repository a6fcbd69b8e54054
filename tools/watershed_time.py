#!/usr/bin/env python3
"""
Device-event times of ddpm3d_basins and ddpm3d_basin_saddles at 130x200x200 and 700x440x440 voxels
of (3.27, 2, 2) mm, on tools/segment_time.py's synthetic target thresholded at about 1 % and about 40 % foreground
(connectivity 26, metrics.segment's labels), with the raw volume and its 8 mm-FWHM Gaussian smoothing as the height.
The C entries are called directly (no ranking, no copy), in alternation with ddpm3d_label_components on the same
volume: --rounds rounds, in each one window of back-to-back calls per entry lasting at least --window seconds;
reported are the median, the minimum and the maximum over the rounds, GB/s of nominal traffic (basins: 20 bytes per
voxel, height and labels read, peaks written, read and written again; saddles: 12 bytes per voxel and 12 per record)
and the ratio to the labelling call.  Beside them: the basins, the records emitted against the unique edges (the
duplication factor), metrics.merge_basins on the host (skipped above --max-merge-edges edges, and where
split_components refuses the basin count), and once per shape scipy.ndimage.label on the host for scale (reported as
absent where scipy is).

    python tools/watershed_time.py [--window 0.2] [--rounds 5] [--no-cpu] [--json profiles/watershed_time.json]
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-denoising-diffusion-model_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from guided_diffusion import _hip as H
from guided_diffusion import metrics
from edt_time import alternate
from segment_time import SHAPES, SHARES, synthetic_target, threshold_for

SPACING = (3.27, 2.0, 2.0)
FWHM = 8.0
CONNECTIVITY = 26
MAX_BASINS = 1 << 20        # split_components' default


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--max-merge-edges", type=int, default=3000000)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("watershed_time: needs a GPU; nothing is measured without one")
    lib = H.load()
    dev = torch.device("cuda:0")
    rows = []

    def row(**kw):
        rows.append(kw)
        print("  ".join("%s=%s" % (k, "%.4g" % v if isinstance(v, float) else v) for k, v in kw.items()), flush=True)

    def med(v):
        return float(np.median(v))

    taps = metrics.gaussian_taps(FWHM, SPACING)
    for shape in SHAPES:
        name = "%dx%dx%d" % shape
        D, Hh, W = shape
        V = D * Hh * W
        vol = synthetic_target(shape, dev)
        smooth = metrics.gaussian_smooth(vol, taps)
        for share in SHARES:
            threshold = threshold_for(vol, share)
            labels, n_comp = metrics.segment(vol, threshold, connectivity=CONNECTIVITY)
            foreground = float((labels > 0).float().mean())
            for height_name, height in (("raw", vol), ("smoothed %g mm" % FWHM, smooth)):
                peaks, n_basins = metrics.basins(height, labels, CONNECTIVITY)
                ws = torch.empty(4, dtype=torch.int32, device=dev)
                status = torch.empty(2, dtype=torch.int32, device=dev)
                _, _, records = metrics._saddle_records(height, labels, peaks, CONNECTIVITY, 0)
                pairs = torch.empty((max(records, 1), 2), dtype=torch.int32, device=dev)
                saddle = torch.empty(max(records, 1), dtype=torch.float32, device=dev)
                out = torch.empty_like(peaks)
                ccl_ws = torch.empty(max(lib.ddpm3d_label_components_workspace_bytes(D, Hh, W), 16) // 4,
                                     dtype=torch.int32, device=dev)

                def call_basins():
                    H.check(lib.ddpm3d_basins(H.ptr(height), H.ptr(labels), CONNECTIVITY, D, Hh, W, H.ptr(out),
                                              H.ptr(ws), 16, H.ptr(status), H.stream()))

                def call_saddles():
                    H.check(lib.ddpm3d_basin_saddles(H.ptr(height), H.ptr(labels), H.ptr(peaks), CONNECTIVITY, D, Hh,
                                                     W, records, H.ptr(pairs), H.ptr(saddle), H.ptr(ws), 16,
                                                     H.ptr(status), H.stream()))

                def call_label():
                    H.check(lib.ddpm3d_label_components(H.ptr(vol), 0, threshold, CONNECTIVITY, D, Hh, W, H.ptr(out),
                                                        H.ptr(ccl_ws), ccl_ws.numel() * 4, H.ptr(status), H.stream()))

                per, reps = alternate({"basins": call_basins, "basin_saddles": call_saddles,
                                       "label_components": call_label}, args.window, args.rounds)
                call_saddles()
                edges = int(metrics.reduce_saddles(pairs[:records], saddle[:records])[0].shape[0])
                common = dict(shape=name, foreground=foreground, height=height_name, components=n_comp,
                              basins=n_basins)
                for entry, nominal in (("basins", 20 * V), ("basin_saddles", 12 * V + 12 * records),
                                       ("label_components", None)):
                    ms = per[entry]
                    r = dict(entry=entry, **common, ms=med(ms), ms_min=min(ms), ms_max=max(ms), rounds=len(ms),
                             calls_per_window=reps[entry])
                    if nominal is not None:
                        r["gb_per_s"] = nominal / med(ms) * 1e-6
                        r["times_label_components"] = med([a / b for a, b in zip(ms, per["label_components"])])
                    if entry == "basin_saddles":
                        r.update(records=records, unique_edges=edges, duplication=records / max(edges, 1))
                    row(**r)
                if n_basins > MAX_BASINS:
                    row(entry="split_components", **common, refused=True,
                        reason="%d basins exceed max_basins = %d: smooth the height first" % (n_basins, MAX_BASINS))
                elif edges > args.max_merge_edges:
                    row(entry="merge_basins (host)", **common, unique_edges=edges, skipped=True)
                else:
                    t0 = time.perf_counter()
                    _, n_after, info = metrics.split_components(labels, height, 0.1, CONNECTIVITY)
                    whole = (time.perf_counter() - t0) * 1e3
                    p, s = metrics.basin_saddles(height, labels, peaks, CONNECTIVITY)
                    flat = peaks.reshape(-1)
                    index = torch.nonzero(flat == torch.arange(V, dtype=torch.int32, device=dev)).reshape(-1)
                    hp = height.reshape(-1).index_select(0, index).cpu().numpy()
                    index, p, s = index.cpu().numpy(), p.cpu().numpy(), s.cpu().numpy()
                    t0 = time.perf_counter()
                    metrics.merge_basins(index, hp, p, s, 0.1)
                    row(entry="merge_basins (host)", **common, unique_edges=edges, prominence=0.1,
                        ms=(time.perf_counter() - t0) * 1e3, split_components_ms=whole, regions=n_after)
                del peaks, pairs, saddle, out
                torch.cuda.empty_cache()
            if not args.no_cpu and share == SHARES[-1]:
                try:
                    from scipy import ndimage
                except ImportError as e:
                    row(entry="scipy.ndimage.label (host, once)", shape=name, absent=True, reason=str(e))
                else:
                    host = (vol > threshold).cpu().numpy()
                    t0 = time.perf_counter()
                    ndimage.label(host, structure=np.ones((3, 3, 3)))
                    row(entry="scipy.ndimage.label (host, once)", shape=name, foreground=foreground,
                        ms=(time.perf_counter() - t0) * 1e3)
                    del host
            del labels
        del vol, smooth
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
