#!/usr/bin/env python3
"""
A/B of kernel forms / launch orders of identical arithmetic, layer by layer, in ONE process
(ddpm3d_conv_desc.kernel_hint): every distinct Winograd-eligible layer shape of the published
architecture, variants interleaved over --rounds rounds.

    python tools/layer_ab.py [--size 64] [--precision f16x3] [--only64] > gpurun_out/layer_ab.txt

--what skip: the ResBlock tails with a 1x1 skip conv that the plan runs fused (ddpm3d_conv3d_skip), each against its
two shipped launches -- the 1x1 conv (+ reduce) into out, then conv2 (+ reduce) with out as its residual -- on the
plan's own buffers.  NOT identical arithmetic (the fp32 sums are ordered differently).  The table fixes the routing
rule (conv3d_params.h ddpm3d_skip_fuse_rule): a level is admitted only if fused was faster in every round.
"""

import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-denoising-diffusion-model_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from guided_diffusion import _hip as H  # noqa: E402
from guided_diffusion import synth  # noqa: E402

IN_MODES = {H.IN_SAME: "same", H.IN_POOL: "pool", H.IN_UP: "up", H.IN_PLANAR2: "planar"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f16", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--only64", action="store_true", help="only the full-resolution layers")
    ap.add_argument("--what", default="order", choices=["order", "issue", "phase", "skip"],
                    help="order: workgroup -> XCD orders; issue: issue orders of a tap (f16x3 Winograd-D kernel); "
                         "phase: the up-sampled-input convs on the 36-tap path against their four-phase form "
                         "(HINT_UP_PHASE: NOT identical arithmetic, the same buffer holds both weight images)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(bench.PUBLISHED, "250", dev)
    model.conv_precision = a.precision
    S, B = a.size, a.batch
    shape = (B, 1, S, S, S)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=3)[0]).to(dev)
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).to(dev)
    t = torch.full((B,), 617, dtype=torch.long, device=dev)
    lib = H.load()
    with torch.no_grad():
        model(x, t, low_res=lr)                       # builds the plan, fills every buffer
    torch.cuda.synchronize()
    plan = model.engine().plan(B, S, S, S)
    ap_what = a.what
    if ap_what == "skip":
        return skip_ab(a, lib, plan, B, S)
    variants = {"order": [("default", 0), ("wstat_off", H.HINT_WSTAT_OFF), ("wstat_on", H.HINT_WSTAT_ON)],
                # issue orders of a tap in the f16x3 Winograd-D kernel (conv3d_wz.h: IL)
                "issue": [("default", 0)] + [("il%d" % il, (il + 1) << H.HINT_WZ_ORDER_SHIFT) for il in (0, 1, 2, 4)],
                "phase": [("taps36", 0), ("phase16", H.HINT_UP_PHASE)]}[ap_what]
    seen = {}
    print("# published architecture, %dx1x%d^3, %s; ms per launch (median of %d rounds x %d launches)"
          % (B, S, a.precision, a.rounds, a.iters))
    print("%-6s %-12s %-12s %2s | %s" % ("input", "Cin->Cout", "DxHxW", "S", "  ".join("%9s" % n for n, _ in variants)))
    for i in sorted(plan.conv_meta):
        tag, fl = plan.conv_meta[i]
        if not any(("_p%d_" % k) in tag for k in (3, 4, 6)):
            continue
        d = plan.steps[i][1][0]._obj
        if a.only64 and d.H != S:
            continue
        planned = d.kernel_hint       # the plan's own hint (HINT_UP_PHASE on the layers that carry the phase image)
        if ap_what == "phase" and not planned & H.HINT_UP_PHASE:
            continue
        keep = 0 if ap_what == "phase" else planned
        key = (d.in_mode, d.Cin, d.Cout, d.D, d.H, d.W, d.res_mode)
        if key in seen:
            continue
        seen[key] = True
        st = H.stream()
        times = {n: [] for n, _ in variants}
        for _ in range(a.rounds):
            for n, hint in variants:
                d.kernel_hint = hint | keep
                H.check(lib.ddpm3d_conv3d(C.byref(d), st))     # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _k in range(a.iters):
                    H.check(lib.ddpm3d_conv3d(C.byref(d), st))
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) / a.iters)
        d.kernel_hint = planned
        med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
        ws = lib.ddpm3d_conv_workspace_bytes(d.N, d.D, d.H, d.W, d.Cin, d.Cout, d.ksize, d.precision)
        split = ws // (d.N * d.D * d.H * d.W * d.Cout * 4) if ws else 1
        best = min(med, key=med.get)
        print("%-6s %-12s %-12s %2d | %s   best %s (%.0f TFLOP/s)" % (
            IN_MODES.get(d.in_mode, "?"), "%d->%d" % (d.Cin, d.Cout), "%dx%dx%d" % (d.D, d.H, d.W), split,
            "  ".join("%9.4f" % med[n] for n, _ in variants), best, fl / med[best] / 1e9))
        if ap_what == "phase":      # every round, so that the spread shows beside the difference
            for n, _ in variants:
                print("#   %-8s rounds: %s" % (n, "  ".join("%.4f" % v for v in times[n])))


def skip_ab(a, lib, plan, B, S):
    """fused ResBlock tails against their two shipped launches, every round printed"""
    print("# published architecture, %dx1x%d^3, %s; ms per ResBlock tail (median of %d rounds x %d launches)"
          % (B, S, a.precision, a.rounds, a.iters))
    print("%-12s %-12s %2s %2s | %9s  %9s   %s" % ("Cx->Cout", "DxHxW", "S", "n", "two_calls", "fused", "verdict"))
    seen, total = {}, {"two_calls": 0.0, "fused": 0.0}
    tails = [(args[0]._obj, args[1]._obj) for fn, args in plan.steps if fn is lib.ddpm3d_conv3d_skip]
    for d, sk in tails:
        key = (sk.C0, sk.C1, d.Cout, d.D, d.H, d.W)
        seen[key] = seen.get(key, 0) + 1
    done = set()
    st = H.stream()
    for d, sk in tails:
        key = (sk.C0, sk.C1, d.Cout, d.D, d.H, d.W)
        if key in done:
            continue
        done.add(key)
        d1 = H.ConvDesc()
        d1.N, d1.D, d1.H, d1.W, d1.Cin, d1.Cout, d1.ksize, d1.in_mode = d.N, d.D, d.H, d.W, sk.C0 + sk.C1, d.Cout, 1, H.IN_SAME
        d1.src0, d1.src1, d1.C0, d1.C1 = sk.src0, sk.src1, sk.C0, sk.C1
        d1.precision, d1.w_packed, d1.bias = H.PREC_F16X3, sk.w_packed, sk.bias
        d1.out, d1.out_layout = d.out, H.OUT_NDHWC
        d1.in_bound, d1.in_bound_count, d1.in_bound_stride = sk.in_bound, sk.in_bound_count, sk.in_bound_stride
        d1.workspace, d1.workspace_bytes = d.workspace, d.workspace_bytes
        if H.conv_plan(d1)[1] > (d.workspace_bytes or 0):
            print("# %s: the 1x1 conv's workspace exceeds the plan's; skipped" % (key,))
            continue
        d2 = H.ConvDesc.from_buffer_copy(d)
        d2.res, d2.res_mode = d.out, H.RES_SAME

        def two_calls():
            H.check(lib.ddpm3d_conv3d(C.byref(d1), st))
            H.check(lib.ddpm3d_conv3d(C.byref(d2), st))

        def fused():
            H.check(lib.ddpm3d_conv3d_skip(C.byref(d), C.byref(sk), st))

        variants = [("two_calls", two_calls), ("fused", fused)]
        times = {n: [] for n, _ in variants}
        for _ in range(a.rounds):
            for n, fn in variants:
                fn()        # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _k in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) / a.iters)
        med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
        every = all(f < t for f, t in zip(times["fused"], times["two_calls"]))
        for n in total:
            total[n] += med[n] * seen[key]
        print("%-12s %-12s %2d %2d | %9.4f  %9.4f   %s" % (
            "%d+%d->%d" % (sk.C0, sk.C1, d.Cout), "%dx%dx%d" % (d.D, d.H, d.W), H.conv_plan(d)[2], seen[key],
            med["two_calls"], med["fused"], "fused in every round" if every else "NOT in every round"))
        for n, _ in variants:
            print("#   %-9s rounds: %s" % (n, "  ".join("%.4f" % v for v in times[n])))
    print("# per forward (medians x occurrences): two_calls %.4f ms, fused %.4f ms" % (total["two_calls"], total["fused"]))


if __name__ == "__main__":
    main()
