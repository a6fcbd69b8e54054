#!/usr/bin/env python3
"""
What keyed sampler noise costs and saves, one process, one device.  Every comparison is against the
un-keyed path of the same run, alternated with it; every row carries the scatter (max - min over the reps) of both.

fill     ddpm3d_noise_fill beside torch.randn into the same buffer at 1 x 96^3, 64 x 96^3 and 1 x 700x440x440:
         device-event ms and GB/s of the bytes written.
step     noise plus update per step: ddpm3d_p_sample_step_keyed beside the noise draw followed by
         ddpm3d_p_sample_step, at the same shapes.  The un-keyed noise is randn_like, and at 64 x 96^3 one th.randn
         per generator of 64 and a th.cat, as scripts/test.py draws it.
loops    p_sample_loop of the published network at 1 and 8 x 96^3, and the joint loop of tools/joint_time.py's
         configuration, with and without a key: host clock around a whole loop ending in a device synchronise, ms per
         step.
memory   the joint loop's peak allocated bytes (torch.cuda.max_memory_allocated) both ways at --mem-draws draws,
         beside what the keyed loop no longer allocates: 4 K V bytes of noise canvases held (V = canvas voxels), up to
         8 K V more while the next ones are drawn and stacked, and 4 bs K r^3 of gathered noise patches.

    python tools/noise_time.py [--reps 5] [--inner 10] [--respacing 10] [--json profiles/noise_time.json]
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
from guided_diffusion import dist_util, joint, patches, synth  # noqa: E402
from guided_diffusion import script_util as su  # noqa: E402
from guided_diffusion.gaussian_diffusion import NoiseKey  # noqa: E402

CASES = [(1, (96, 96, 96)), (64, (96, 96, 96)), (1, (700, 440, 440))]


def alternated(fns, reps, inner):
    """{name: [ms per call]} of device-event pairs around `inner` calls, the functions taking turns within each rep,
    after two warm-up calls each"""
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / inner)
    return ms


def summary(ms):
    return {"ms": float(np.median(ms)), "scatter_ms": float(max(ms) - min(ms)), "all_ms": [float(v) for v in ms]}


def kernel_rows(args, dev):
    lib = H.load()
    diff = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="10")
    coef = diff._device_state(dev)["coef"]
    flags = diff._flags(True)
    fill_rows, step_rows = [], []
    for N, dhw in CASES:
        voxels = dhw[0] * dhw[1] * dhw[2]
        shape = (N, 1) + dhw
        inner = args.inner if N * voxels < 10 ** 7 else 2
        key = NoiseKey(10, [dist_util.noise_stream(i, 0) for i in range(N)], device=dev)
        buf = torch.empty(shape, device=dev)
        desc = key.desc(1)

        def keyed_fill():
            H.check(lib.ddpm3d_noise_fill(desc, N, voxels, H.ptr(buf), H.stream()))

        def torch_fill():
            torch.randn(shape, out=buf)

        ms = alternated({"keyed": keyed_fill, "torch": torch_fill}, args.reps, inner)
        nbytes = 4.0 * N * voxels
        row = dict(shape="%dx%dx%dx%d" % ((N,) + dhw), mb=nbytes * 1e-6, keyed=summary(ms["keyed"]),
                   torch=summary(ms["torch"]))
        for side in ("keyed", "torch"):
            row[side]["gb_per_s"] = nbytes / row[side]["ms"] * 1e-6
        fill_rows.append(row)
        print("fill  %-16s keyed %8.4f ms (%7.1f GB/s)  torch.randn %8.4f ms (%7.1f GB/s)"
              % (row["shape"], row["keyed"]["ms"], row["keyed"]["gb_per_s"], row["torch"]["ms"],
                 row["torch"]["gb_per_s"]), flush=True)

        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(shape, device=dev, generator=gen)
        mo = torch.randn((N, 2) + dhw, device=dev, generator=gen)
        mo[:, 1].clamp_(-1, 1)
        sample, x0 = torch.empty_like(x), torch.empty_like(x)
        t = torch.full((N,), 5, dtype=torch.int64, device=dev)
        gens = [dist_util.volume_generator(i, seed=10, device=dev) for i in range(N)]

        def keyed_step():
            H.check(lib.ddpm3d_p_sample_step_keyed(H.ptr(mo), H.ptr(x), desc, H.ptr(coef), H.ptr(t), N, voxels, flags,
                                                   H.ptr(sample), H.ptr(x0), H.stream()))

        def unkeyed_step():
            if N == 1:
                z = torch.randn_like(x)
            else:
                z = torch.cat([torch.randn(1, 1, *dhw, device=dev, generator=g) for g in gens])
            H.check(lib.ddpm3d_p_sample_step(H.ptr(mo), H.ptr(x), H.ptr(z), H.ptr(coef), H.ptr(t), N, voxels, flags,
                                             H.ptr(sample), H.ptr(x0), H.stream()))

        ms = alternated({"keyed": keyed_step, "unkeyed": unkeyed_step}, args.reps, inner)
        row = dict(shape="%dx%dx%dx%d" % ((N,) + dhw),
                   unkeyed_noise="randn_like" if N == 1 else "%d generators, one th.randn each, th.cat" % N,
                   keyed=summary(ms["keyed"]), unkeyed=summary(ms["unkeyed"]))
        step_rows.append(row)
        print("step  %-16s keyed %8.4f ms  noise + un-keyed %8.4f ms (%s)"
              % (row["shape"], row["keyed"]["ms"], row["unkeyed"]["ms"], row["unkeyed_noise"]), flush=True)
        del buf, x, mo, sample, x0
        torch.cuda.empty_cache()
    return fill_rows, step_rows


def host_timed(fns, reps, steps):
    """{name: [ms per step]} of whole loops on the host clock, each ending in a device synchronise, taking turns"""
    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for fn in fns.values():
        once(fn)
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ms[name].append(once(fn))
    return ms


def verdict(row):
    """the issue's only performance condition: keyed not slower than un-keyed by more than the un-keyed scatter"""
    row["difference_ms_per_step"] = row["keyed"]["ms"] - row["unkeyed"]["ms"]
    row["within_unkeyed_scatter"] = bool(row["difference_ms_per_step"] <= row["unkeyed"]["scatter_ms"])
    return row


def loop_rows(args, dev):
    model, diff, _ = bench.build_model(bench.PUBLISHED, args.respacing, dev)
    T = diff.num_timesteps
    rows = []
    for B in (1, 8):
        shape = (B, 1, 96, 96, 96)
        kw = {"low_res": torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)}
        key = NoiseKey(10, [dist_util.noise_stream(i, 0) for i in range(B)], device=dev)
        ms = host_timed({"unkeyed": lambda: diff.p_sample_loop(model, shape, model_kwargs=kw),
                         "keyed": lambda: diff.p_sample_loop(model, shape, model_kwargs=kw, noise_key=key)},
                        args.reps, T)
        rows.append(verdict(dict(loop="p_sample_loop", shape=list(shape), steps=T, reps=args.reps,
                                 unkeyed_noise="randn_like", unkeyed=summary(ms["unkeyed"]),
                                 keyed=summary(ms["keyed"]))))
        print("loop  p_sample_loop %dx96^3: %.3f ms/step un-keyed (scatter %.3f), %.3f keyed"
              % (B, rows[-1]["unkeyed"]["ms"], rows[-1]["unkeyed"]["scatter_ms"], rows[-1]["keyed"]["ms"]), flush=True)
    del model
    torch.cuda.empty_cache()
    return rows


def joint_rows(args, dev):
    shape_dhw, res, steps = (130, 200, 200), 96, 4                          # tools/joint_time.py's configuration
    model, diff, _ = bench.build_model(dict(bench.PUBLISHED, large_size=res, small_size=res), str(steps), dev)
    vol = synth.synth_low_res(shape_dhw, seed=1234)
    geom = patches.joint_geometry(shape_dhw, res)
    P, V = geom.n_patches, int(np.prod(geom.canvas))

    def run(K, keyed):
        kw = dict(noise_key=joint.draw_key(10, K, dev)) if keyed else {}
        return joint.sample_loop(diff, model, vol, geom, batch_size=1, num_draws=K, device=dev, **kw)

    ms = host_timed({"unkeyed": lambda: run(1, False), "keyed": lambda: run(1, True)}, max(3, args.reps // 2), steps)
    time_row = verdict(dict(loop="joint.sample_loop", volume_dhw=list(shape_dhw), res=res, patches=P, batch_size=1,
                            draws=1, steps=steps, unkeyed_noise="one generator per draw, whole canvases, gathered",
                            unkeyed=summary(ms["unkeyed"]), keyed=summary(ms["keyed"])))
    print("loop  joint %s: %.3f ms/step un-keyed (scatter %.3f), %.3f keyed"
          % (shape_dhw, time_row["unkeyed"]["ms"], time_row["unkeyed"]["scatter_ms"], time_row["keyed"]["ms"]),
          flush=True)

    K = args.mem_draws
    peaks = {}
    for name, keyed in (("unkeyed", False), ("keyed", True)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        run(K, keyed)
        torch.cuda.synchronize()
        peaks[name] = dict(peak_bytes=int(torch.cuda.max_memory_allocated(dev)), allocated_before=int(base))
    r3 = res ** 3
    mem_row = dict(volume_dhw=list(shape_dhw), canvas=list(geom.canvas), patches=P, draws=K, batch_size=1, steps=steps,
                   unkeyed=peaks["unkeyed"], keyed=peaks["keyed"],
                   saved_bytes=peaks["unkeyed"]["peak_bytes"] - peaks["keyed"]["peak_bytes"],
                   formula=dict(held_noise_canvases_4KV=4 * K * V, gathered_noise_patches_4bsKr3=4 * K * r3,
                                transient_while_drawing_up_to_8KV=8 * K * V,
                                updated_patches_unchanged_8PKr3=8 * P * K * r3))
    print("mem   joint K=%d: peak %.1f MB un-keyed, %.1f MB keyed (saved %.1f MB; 4KV + 4 bs K r^3 = %.1f MB held, up to "
          "%.1f MB more while drawing)" % (K, peaks["unkeyed"]["peak_bytes"] * 1e-6, peaks["keyed"]["peak_bytes"] * 1e-6,
                                          mem_row["saved_bytes"] * 1e-6, (4 * K * V + 4 * K * r3) * 1e-6,
                                          8 * K * V * 1e-6), flush=True)
    return time_row, mem_row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--respacing", default="10")
    ap.add_argument("--mem-draws", type=int, default=4)
    ap.add_argument("--no-loops", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_time: no GPU visible (there is nothing to time on the host)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps}
    res["fill"], res["step"] = kernel_rows(args, dev)
    if not args.no_loops:
        res["loops"] = loop_rows(args, dev)
        joint_time, res["joint_memory"] = joint_rows(args, dev)
        res["loops"].append(joint_time)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
