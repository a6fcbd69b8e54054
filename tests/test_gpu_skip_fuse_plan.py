"""
Routing of ddpm3d_conv3d_skip by the planner and its two replayers, on the published network in the f16x3 mode: the
plan (csrc/unet_plan.hip), replayed from Python (engine.py) and by the library, runs the tail of every ResBlock with a
1x1 skip conv as ONE step wherever the library takes its fused form (ddpm3d_conv_skip_fused) and as the two shipped
steps elsewhere, and the two forwards are bitwise equal; DDPM3D_SKIP_FUSE=0 restores the two-step list.  The fused and the two-step
forwards differ in rounding only: by at most twice the two-step forward's own distance from the exact-f32 forward of
the same inputs.
"""

import ctypes as C
import os

import pytest
import torch

import test_gpu_model as M

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 32, 32), (1, 1, 64, 64, 64)]


def _forward(model, shape, native):
    x, lr = M.inputs(shape)
    model.native_plan = native
    with torch.no_grad():
        return model(x.cuda(), torch.tensor([251]).cuda(), low_res=lr.cuda()).cpu()


def _steps(model, shape):
    """the Python plan's steps as (entry name, args)"""
    eng = model.engine()
    plan = eng.plan(*[shape[0]] + list(shape[2:]))
    name = lambda fn: ("ddpm3d_conv3d" if fn is eng.lib.ddpm3d_conv3d else
                       "ddpm3d_conv3d_skip" if fn is eng.lib.ddpm3d_conv3d_skip else "other")
    return eng, [(name(fn), a) for fn, a in plan.steps]


@pytest.fixture(scope="module")
def runs():
    """per shape: forwards of the Python and the native plan with the default routing and under DDPM3D_SKIP_FUSE=0,
    the exact-f32 forward, and the two Python step lists"""
    keep = os.environ.pop("DDPM3D_SKIP_FUSE", None)
    out = {}
    try:
        model, _ = M.build(M.PUBLISHED, "10", precision="f16x3")
        for s in SHAPES:
            out[s] = dict(py=_forward(model, s, False), nat=_forward(model, s, True))
            out[s]["eng"], out[s]["steps"] = _steps(model, s)
        os.environ["DDPM3D_SKIP_FUSE"] = "0"
        model0, _ = M.build(M.PUBLISHED, "10", precision="f16x3")
        for s in SHAPES:
            out[s].update(py0=_forward(model0, s, False), nat0=_forward(model0, s, True))
            out[s]["steps0"] = _steps(model0, s)[1]
        out["keep"] = (model, model0)
    finally:
        os.environ.pop("DDPM3D_SKIP_FUSE", None)
        if keep is not None:
            os.environ["DDPM3D_SKIP_FUSE"] = keep
    model32, _ = M.build(M.PUBLISHED, "10", precision="f32")
    for s in SHAPES:
        out[s]["f32"] = _forward(model32, s, False)
    del model32
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["8x32x32", "64x64x64"])
def test_both_planners_fuse_where_the_library_does_and_the_override_restores(runs, shape):
    import guided_diffusion._hip as H
    r = runs[shape]
    eng, steps, steps0 = r["eng"], r["steps"], r["steps0"]
    lib = eng.lib
    n_skip = sum(1 for k in eng.conv if k.endswith(".skip_connection"))
    assert n_skip == 18
    fused = [a for n, a in steps if n == "ddpm3d_conv3d_skip"]
    # a fused step is conv2's descriptor (no residual, SiLU prologue, Winograd-D f16x3) plus the skip conv, and the
    # library says it fuses; its statistics rows / workspace are conv2's own (the plan sized them with conv_plan)
    for a in fused:
        d, sk = a[0]._obj, a[1]._obj
        assert d.precision == H.PREC_F16X3_WZ and d.res_mode == H.RES_NONE and d.act == H.ACT_SILU and d.ksize == 3
        assert lib.ddpm3d_conv_skip_fused(C.byref(d), C.byref(sk)) == 1
        assert d.stats_rows == H.conv_plan(d)[0]
    # every other ResBlock with a skip conv keeps its two steps, and the library would not fuse it
    convs = [a[0]._obj for n, a in steps if n == "ddpm3d_conv3d"]
    pairs = [(d1, d2) for d1, d2 in zip(convs, convs[1:])
             if d1.ksize == 1 and not d1.aff_a and not d1.stats and d2.ksize == 3 and d2.res_mode == H.RES_SAME
             and d2.res == d1.out and d2.out == d1.out]
    assert len(fused) + len(pairs) == n_skip
    for d1, d2 in pairs:
        sk = H.ConvSkip()
        sk.src0, sk.src1, sk.C0, sk.C1, sk.w_packed, sk.bias = d1.src0, d1.src1, d1.C0, d1.C1, d1.w_packed, d1.bias
        sk.in_bound, sk.in_bound_count, sk.in_bound_stride = d1.in_bound, d1.in_bound_count, d1.in_bound_stride
        d = H.ConvDesc.from_buffer_copy(d2)
        d.res, d.res_mode = 0, H.RES_NONE
        assert lib.ddpm3d_conv_skip_fused(C.byref(d), C.byref(sk)) == 0
    print("%s: %d of %d skip ResBlocks run fused" % (shape, len(fused), n_skip))
    assert fused, "the rule admits no level at all"
    # ---- DDPM3D_SKIP_FUSE=0: no fused step; the list is the fused one with each fused step as its two convs
    assert not any(n == "ddpm3d_conv3d_skip" for n, _ in steps0)
    expand = []
    for n, _ in steps:
        expand += ["ddpm3d_conv3d", "ddpm3d_conv3d"] if n == "ddpm3d_conv3d_skip" else [n]
    assert [n for n, _ in steps0] == expand
    # ---- the two replayers agree bit for bit under either routing; the routings differ in rounding only
    assert torch.isfinite(r["py"]).all()
    assert torch.equal(r["py"], r["nat"]) and torch.equal(r["py0"], r["nat0"])
    assert not torch.equal(r["py"], r["py0"])
    top = float(r["py0"].abs().max())
    rel = float((r["py"] - r["py0"]).abs().max()) / top
    own = float((r["py0"] - r["f32"]).abs().max()) / top
    print("%s: fused vs two-step forward: max rel difference %.3g; two-step vs exact f32: %.3g" % (shape, rel, own))
    assert rel <= 2 * own
