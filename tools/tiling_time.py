#!/usr/bin/env python3
"""
Time of the two sliding-tiling kernels (ddpm3d_tiles_gather / ddpm3d_tiles_blend), one process, one
device: ms per call and GB/s of the bytes the call has to move (gather: the patches read and written; blend: the
patches read, the canvas written).

Geometry 1, 200x200x130 at 96^3 (18 patches, K = 1): the same starts through the fixed-grid entries
(ddpm3d_joint_gather / ddpm3d_joint_blend) and the tiles entries, alternated call by call after a warm-up; reported
are the medians, their ratio and the run-to-run scatter ((max - min) / median over the passes' medians) of the
fixed-grid entries, which is what the ratio has to be read against.
Geometry 2, 700x440x440 at 96^3, overlap 44 (832 patches, K = 1): the tiles entries alone (the fixed-grid entries
refuse it), beside the traffic floor.

Every call is timed with device events around one launch sequence.  Prints one JSON line and writes it to --out.

    python tools/tiling_time.py [--reps 20] [--passes 5] [--skip-whole-body] [--out profiles/tiling_time.json]
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-denoising-diffusion-model_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from guided_diffusion import joint, patches  # noqa: E402


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(fns, reps, passes):
    """{name: [median ms of each pass]}; within a pass the functions take turns call by call."""
    out = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(passes):
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                t[k].append(_ms(fn))
        for k in fns:
            out[k].append(statistics.median(t[k]))
    return out


def _summary(times, nbytes):
    med = statistics.median(times)
    return dict(ms=med, gb_per_s=nbytes / med / 1e6, scatter=(max(times) - min(times)) / med, passes=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--skip-whole-body", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiling_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiling_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    rec = dict(tool="tiling_time", device=torch.cuda.get_device_name(0), reps=a.reps, passes=a.passes)

    # ---- 18 patches: old and new entries on the same starts
    res = 96
    old = patches.joint_geometry((130, 200, 200), res)
    new = patches.joint_geometry((130, 200, 200), res, min_overlap=44)
    assert old.grid == new.grid
    P, r3, vox = old.n_patches, res ** 3, old.canvas[0] * old.canvas[1] * old.canvas[2]
    canvas = torch.randn((1,) + old.canvas, device=dev)
    rows = torch.randn((P, 1, res, res, res), device=dev)
    g_out, b_out = torch.empty_like(rows), torch.empty_like(canvas)
    t = _alternate({
        "joint_gather": lambda: joint.gather(canvas, old, out=g_out),
        "tiles_gather": lambda: joint.gather(canvas, new, out=g_out),
        "joint_blend": lambda: joint.blend(rows, old, out=b_out),
        "tiles_blend": lambda: joint.blend(rows, new, out=b_out),
    }, a.reps, a.passes)
    gather_bytes, blend_bytes = 2 * P * r3 * 4, (P * r3 + vox) * 4
    small = {k: _summary(v, gather_bytes if "gather" in k else blend_bytes) for k, v in t.items()}
    for op in ("gather", "blend"):
        o, n = small["joint_" + op], small["tiles_" + op]
        small[op + "_ratio_new_over_old"] = n["ms"] / o["ms"]
        small[op + "_within_old_scatter"] = n["ms"] <= o["ms"] * (1 + o["scatter"])
    rec["fixed_grid_18_patches"] = dict(volume_dhw=[130, 200, 200], res=res, patches=P, gather_mb=gather_bytes / 1e6,
                                        blend_mb=blend_bytes / 1e6, **small)
    del canvas, rows, g_out, b_out

    # ---- whole body: 832 patches
    if not a.skip_whole_body:
        geom = patches.joint_geometry((700, 440, 440), res, min_overlap=44)
        P, vox = geom.n_patches, geom.canvas[0] * geom.canvas[1] * geom.canvas[2]
        canvas = torch.randn((1,) + geom.canvas, device=dev)
        rows = torch.empty((P, 1, res, res, res), device=dev)
        b_out = torch.empty_like(canvas)
        t = _alternate({
            "tiles_gather": lambda: joint.gather(canvas, geom, out=rows),
            "tiles_blend": lambda: joint.blend(rows, geom, out=b_out),
        }, max(3, a.reps // 4), a.passes)
        gather_bytes, blend_bytes = 2 * P * r3 * 4, (P * r3 + vox) * 4
        rec["whole_body_832_patches"] = dict(
            volume_dhw=[700, 440, 440], res=res, overlap=44, patches=P,
            per_axis=[len(geom.z_starts), len(geom.x_starts), len(geom.y_starts)],
            gather_gb=gather_bytes / 1e9, blend_read_gb=P * r3 * 4 / 1e9, blend_written_gb=vox * 4 / 1e9,
            tiles_gather=_summary(t["tiles_gather"], gather_bytes),
            tiles_blend=_summary(t["tiles_blend"], blend_bytes))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
