"""
Routing of the phase form (DDPM3D_HINT_UP_PHASE) by the planner and its two replayers: the plan (csrc/unet_plan.hip),
replayed from Python (engine.py) and by the library, gives conv1 of every up-ResBlock -- and nothing else -- the phase
image and the hint, and the two forwards are bitwise equal; DDPM3D_UP_PHASE=0 restores the 36-tap routing.
"""

import ctypes as C

import pytest
import torch

import test_gpu_model as M

pytestmark = pytest.mark.gpu

SHAPE = (1, 1, 8, 32, 32)     # up-ResBlock outputs 8x4x4 (falls back: 2x2 source), 8x8x8, 8x16x16, 8x32x32


def _forward(model, native):
    x, lr = M.inputs(SHAPE)
    model.native_plan = native
    with torch.no_grad():
        return model(x.cuda(), torch.tensor([251]).cuda(), low_res=lr.cuda()).cpu()


def _hinted(model):
    """(prefix of the conv's layer, descriptor) of every conv step of the Python plan that carries the hint"""
    import guided_diffusion._hip as H
    eng = model.engine()
    plan = eng.plan(*[SHAPE[0]] + list(SHAPE[2:]))
    descs = [a[0]._obj for fn, a in plan.steps if fn is eng.lib.ddpm3d_conv3d]
    return eng, descs, [d for d in descs if d.kernel_hint & H.HINT_UP_PHASE]


def test_both_planners_route_the_phase_form_and_the_override_restores(monkeypatch):
    import guided_diffusion._hip as H
    monkeypatch.delenv("DDPM3D_UP_PHASE", raising=False)
    model, _ = M.build(M.PUBLISHED, "10", precision="f16x3")
    y_py, y_nat = _forward(model, False), _forward(model, True)
    eng, descs, hinted = _hinted(model)
    assert eng.native_plan and eng.native_plans
    # the hint sits on the up-sampled-input Winograd-D convs and on nothing else: conv1 of the four up-ResBlocks
    assert len(hinted) == 4
    assert all(d.in_mode == H.IN_UP and d.precision == H.PREC_F16X3_WZ for d in hinted)
    assert not any(d.in_mode == H.IN_UP and not (d.kernel_hint & H.HINT_UP_PHASE) for d in descs)
    up1 = [k for k, pc in eng.conv.items() if pc.wz is not None and pc.wz.up_phase]
    assert len(up1) == 4 and all(k.endswith(".in_layers.2") for k in up1)
    # precision, kernel family and the plan's statistics rows / workspace are those of the unhinted descriptor
    for d in hinted:
        with_hint = H.conv_plan(d)
        name, name0 = C.create_string_buffer(64), C.create_string_buffer(64)
        H.check(eng.lib.ddpm3d_conv_kernel_family(C.byref(d), name, 64))
        d.kernel_hint = 0
        H.check(eng.lib.ddpm3d_conv_kernel_family(C.byref(d), name0, 64))
        assert with_hint == H.conv_plan(d) and name.value == name0.value
        d.kernel_hint = H.HINT_UP_PHASE
    assert torch.isfinite(y_py).all() and torch.equal(y_py, y_nat)

    monkeypatch.setenv("DDPM3D_UP_PHASE", "0")
    model0, _ = M.build(M.PUBLISHED, "10", precision="f16x3")
    y0_py, y0_nat = _forward(model0, False), _forward(model0, True)
    eng0, _, hinted0 = _hinted(model0)
    assert not hinted0 and not any(pc.wz is not None and pc.wz.up_phase for pc in eng0.conv.values())
    assert torch.equal(y0_py, y0_nat)
    # the two routings differ in rounding only
    assert not torch.equal(y_py, y0_py)
    rel = float((y_py - y0_py).abs().max() / y0_py.abs().max())
    print("phase vs 36-tap routing, whole forward: max rel difference %.3g" % rel)
    assert rel < 1e-4
