#!/usr/bin/env python3
"""
Cost of the uncertainty maps beside the sampling they summarise, one process, one device: ddpm3d_draw_stitch per
patch origin (96^3 patches, K draws, the origins of a whole-body volume), ddpm3d_draw_moments once over that volume,
and one sampler step (UNet forward + DDPM update) of the published network on the same N = K batch (one patch x K
draws).  Device events around each timed region, after warm-up.  The share is (stitch per origin x origins +
moments) / (step x steps x origins), the sampling of every origin at --steps steps.  Prints one JSON line.

    python tools/uncertainty_time.py [--draws 8] [--volume 700,440,440] [--steps 250] [--reps 5] [--out u.json]
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-denoising-diffusion-model_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from guided_diffusion import patches, synth, uncertainty  # noqa: E402


def _ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=8)
    ap.add_argument("--volume", default="700,440,440", help="D,H,W of the stitched volume")
    ap.add_argument("--res", type=int, default=96)
    ap.add_argument("--steps", type=int, default=250, help="sampler steps per patch the share is taken against")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uncertainty_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    K, res = a.draws, a.res
    shape_dhw = tuple(int(v) for v in a.volume.split(","))
    grid = patches.patch_grid(shape_dhw, res)
    samples = torch.randn(K, 1, res, res, res, device=dev)

    st = uncertainty.DrawStitcher(shape_dhw, res, K, dev)
    n_added = [0]

    def stitch_all():              # the same origins again under ascending indices: the accumulators just grow
        for origin in grid:
            st.add(n_added[0], samples, origin)
            n_added[0] += 1

    stitch_all()
    stitch_ms = _ms(stitch_all, a.reps) / len(grid)
    st.finish()
    moments_ms = _ms(st.finish, a.reps)
    voxels = st.wsum.numel()
    del st
    torch.cuda.empty_cache()

    # one sampler step at N = K: a 2-step schedule, timed whole and halved (forward + update + noise draw per step)
    model, diff, _ = bench.build_model(bench.PUBLISHED, "2", dev)
    shape = (K, 1, res, res, res)
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)
    noise = torch.randn(shape, device=dev)

    def sample():
        diff.p_sample_loop(model, shape, noise, model_kwargs={"low_res": lr})

    sample()
    step_ms = _ms(sample, a.reps) / diff.num_timesteps

    sampling_ms = step_ms * a.steps * len(grid)
    maps_ms = stitch_ms * len(grid) + moments_ms
    rec = dict(tool="uncertainty_time", draws=K, res=res, volume_dhw=list(shape_dhw), voxels=voxels,
               origins=len(grid), stitch_ms_per_origin=stitch_ms, moments_ms=moments_ms,
               step_ms_at_n=step_ms, n=K, steps=a.steps, sampling_ms=sampling_ms, maps_ms=maps_ms,
               share_of_sampling=maps_ms / sampling_ms,
               moments_gbps=(K + 3) * voxels * 4 / (moments_ms * 1e6),
               # nominal bytes of an uncropped origin: samples and window read, accumulators and weights read + written
               stitch_gbps=(12 * K + 16) * res ** 3 / (stitch_ms * 1e6))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
