#!/usr/bin/env python3
"""
Cost of joint patch sampling beside the independent loop it replaces, one process, one device: ms per reverse step of
the whole volume (all patches: forwards, step kernels and, for the joint loop, two gathers per batch and two blends
per step) with the published network on synthetic weights.  The independent side is one p_sample_loop per batch of
patches with randn_like noise (scripts/test.py's default path, but for its per-patch generators).  Both run the same
--steps-step schedule over the same patches at the same batch size, alternating, after one warm-up pass each; a pass
is timed by the host clock around work that ends in a device synchronise.  Reported: the median ms per step of
either loop, their ratio, and the scatter of the independent loop's own repeats ((max - min) / median), which is what the ratio has to be read
against.  Prints one JSON line.

    python tools/joint_time.py [--volume 130,200,200] [--res 96] [--batch_size 1] [--steps 4] [--reps 5]
                               [--arch published|tiny] [--out j.json]
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-denoising-diffusion-model_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from guided_diffusion import joint, patches, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", default="130,200,200", help="D,H,W of the volume")
    ap.add_argument("--res", type=int, default=96)
    ap.add_argument("--batch_size", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4, help="reverse steps per timed pass")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--arch", default="published", choices=["published", "tiny"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("joint_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    shape_dhw = tuple(int(v) for v in a.volume.split(","))
    res, bs = a.res, a.batch_size
    arch = dict(bench.PUBLISHED if a.arch == "published" else bench.TINY, large_size=res, small_size=res)
    model, diff, _ = bench.build_model(arch, str(a.steps), dev)
    vol = synth.synth_low_res(shape_dhw, seed=1234)
    geom = patches.joint_geometry(shape_dhw, res)
    low_res, grid = patches.split_volume(vol, res)
    conds = [torch.from_numpy(low_res[i:i + bs]).to(dev) for i in range(0, len(grid), bs)]

    def independent():
        for cond in conds:
            shape = tuple(cond.shape)
            diff.p_sample_loop(model, shape, torch.randn(shape, device=dev), model_kwargs={"low_res": cond})

    def jointly():
        joint.sample_loop(diff, model, vol, geom, batch_size=bs, device=dev)

    def ms_per_step(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / diff.num_timesteps

    independent()
    jointly()
    ind, jnt = [], []
    for _ in range(a.reps):
        ind.append(ms_per_step(independent))
        jnt.append(ms_per_step(jointly))
    ind_ms, jnt_ms = statistics.median(ind), statistics.median(jnt)
    r3 = res ** 3
    voxels = geom.canvas[0] * geom.canvas[1] * geom.canvas[2]
    # bytes the joint loop adds per step: x_t and noise gathered (patch read + written), two blends (patches read,
    # canvas written)
    extra_bytes = 4 * (2 * 2 * len(grid) * r3 + 2 * (len(grid) * r3 + voxels))
    rec = dict(tool="joint_time", arch=a.arch, volume_dhw=list(shape_dhw), res=res, patches=len(grid), batch_size=bs,
               steps_per_pass=diff.num_timesteps, reps=a.reps,
               independent_ms_per_step=ind_ms, joint_ms_per_step=jnt_ms, ratio=jnt_ms / ind_ms,
               independent_scatter=(max(ind) - min(ind)) / ind_ms, joint_scatter=(max(jnt) - min(jnt)) / jnt_ms,
               independent_all=ind, joint_all=jnt, joint_extra_mb_per_step=extra_bytes / 1e6)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
