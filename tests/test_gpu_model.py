"""
Whole-network and whole-sampler parity on the GPU: the HIP engine behind the
reference's API vs (a) the committed golden outputs of the reference itself
and (b) the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): 1e-3 relative, fp32.  Observed differences
are summation-order rounding, so single forwards are held to 1e-4.
"""

import numpy as np
import pytest
import torch

from conftest import rel_err, rel_err_per_channel
from guided_diffusion import script_util as su
from guided_diffusion import synth

pytestmark = pytest.mark.gpu

PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True,
                 use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)


def build(over, resp="", precision=None):
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(over)
    fl["timestep_respacing"] = resp
    model, diff = su.sr_create_model_and_diffusion(**fl)
    if precision is not None:
        model.conv_precision = precision
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape))) for k, v in sd.items()})
    model.to("cuda").eval()
    return model, diff


def inputs(shape):
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=3)[0])
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234))
    return x, lr


@pytest.mark.parametrize("tag,over,shape,t", [
    ("tiny_8x16x16", {}, (2, 1, 8, 16, 16), [37, 999]),
    ("tiny_32", {}, (1, 1, 32, 32, 32), [500]),
    ("tiny_odd", {}, (1, 1, 5, 48, 16), [3]),
    ("tiny_additive", dict(use_scale_shift_norm=False), (1, 1, 4, 16, 16), [5]),
    ("tiny_nosigma", dict(learn_sigma=False), (1, 1, 4, 16, 16), [5]),
    ("tiny_ls64", dict(large_size=64), (1, 1, 4, 16, 16), [5]),
    # conv Downsample / Upsample between levels (unet.py:81-140), the factory's default flag
    ("tiny_convresample", dict(resblock_updown=False), (1, 1, 4, 16, 16), [5]),
])
def test_unet_forward_vs_reference_golden(golden, tag, over, shape, t):
    model, _ = build(dict(TINY, **over))
    x, lr = inputs(shape)
    with torch.no_grad():
        y = model(x.cuda(), torch.tensor(t[:shape[0]]).cuda(), low_res=lr.cuda())
    ref = golden("unet_forward.npz")[tag]
    assert tuple(y.shape) == ref.shape
    assert rel_err(y.cpu().numpy(), ref) < 1e-4, tag


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_unet_forward_published_architecture(golden, precision):
    """206 964 610-parameter network with mult (1,1,2,3,4) / 2 res blocks, at 1x1x8x32x32:
    pins the decoder's channel bookkeeping and every tile configuration it uses, in both
    arithmetic modes of the 3x3x3 convolutions at the same tolerance."""
    model, _ = build(PUBLISHED, precision=precision)
    x, lr = inputs((1, 1, 8, 32, 32))
    with torch.no_grad():
        y = model(x.cuda(), torch.tensor([251]).cuda(), low_res=lr.cuda())
    assert rel_err(y.cpu().numpy(), golden("unet_forward.npz")["published_8x32x32"]) < 1e-4


def test_unet_with_level_attention_vs_reference_golden(golden):
    """attention_resolutions='8,4' on the factory's (_noatt) class: AttentionBlocks after the
    ResBlocks at ds 4 and 8 (2 and 3 heads of 32 channels), encoder and decoder."""
    model, _ = build(dict(TINY, large_size=32, attention_resolutions="8,4", num_head_channels=32))
    x, lr = inputs((1, 1, 8, 32, 32))
    with torch.no_grad():
        y = model(x.cuda(), torch.tensor([10]).cuda(), low_res=lr.cuda())
    assert rel_err(y.cpu().numpy(), golden("unet_forward.npz")["tiny_attn"]) < 1e-4


def test_unet_with_mid_block_attention_vs_reference_golden(golden):
    """SuperResModel / UNetModel (unet.py:396-716, 1655-1673): the variant north_star names,
    with the AttentionBlock between the two middle ResBlocks.  Built directly, as the golden was
    (sr_create_model only returns the _noatt class)."""
    from guided_diffusion.unet import SuperResModel
    model = SuperResModel(image_size=32, in_channels=1, model_channels=32, out_channels=2, num_res_blocks=1,
                          attention_resolutions=(1000,), channel_mult=(1, 1, 2, 3, 4), dims=3,
                          num_head_channels=32, use_scale_shift_norm=True, resblock_updown=True)
    sd = model.state_dict()
    assert "middle_block.1.qkv.weight" in sd and "middle_block.2.in_layers.2.weight" in sd
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape))) for k, v in sd.items()})
    model.to("cuda").eval()
    x, lr = inputs((1, 1, 4, 32, 32))
    with torch.no_grad():
        y = model(x.cuda(), torch.tensor([77]).cuda(), low_res=lr.cuda())
    assert rel_err(y.cpu().numpy(), golden("unet_forward.npz")["tiny_midattn"]) < 1e-4


def test_unet_forward_vs_oracle_layerwise():
    """Same weights through oracle/unet_ref.py; also a size no golden covers."""
    from oracle import unet_ref
    model, _ = build(TINY)
    cfg = unet_ref.sr_config(**TINY)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    x, lr = inputs((2, 1, 6, 32, 48))
    t = torch.tensor([0, 640])
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, cfg, x, t, lr)
        y = model(x.cuda(), t.cuda(), low_res=lr.cuda())
    assert rel_err(y.cpu().numpy(), ref.numpy()) < 1e-4


@pytest.mark.parametrize("tag,over,shape,resp,kind,eta,kw", [
    ("ddpm10_32", {}, (1, 1, 32, 32, 32), "10", "ddpm", 0.0, {}),
    ("ddim10_8x16x16", {}, (2, 1, 8, 16, 16), "ddim10", "ddim", 0.0, {}),
    ("ddim10_eta_8x16x16", {}, (1, 1, 8, 16, 16), "ddim10", "ddim", 0.5, {}),
    ("ddpm10_nosigma", dict(learn_sigma=False), (1, 1, 4, 16, 16), "10", "ddpm", 0.0, {}),
    ("ddpm10_noclip", {}, (1, 1, 4, 16, 16), "10", "ddpm", 0.0, dict(clip_denoised=False)),
    ("ddpm10_xstart", dict(predict_xstart=True), (1, 1, 4, 16, 16), "10", "ddpm", 0.0, {}),
])
def test_sampler_loops_vs_reference_golden(golden, tag, over, shape, resp, kind, eta, kw):
    """BASELINE config 1 (tiny UNet, 1x32^3, 10 steps) end to end and its variants, with the
    reference's noise draws injected in order."""
    model, diff = build(dict(TINY, **over), resp)
    T = diff.num_timesteps
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, T + 1, seed=10)]
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).cuda()
    trace = []
    if kind == "ddpm":
        gen = diff.p_sample_loop_progressive(model, shape, draws[0], model_kwargs={"low_res": lr},
                                             step_noise=draws[1:], **kw)
    else:
        gen = diff.ddim_sample_loop_progressive(model, shape, draws[0], eta=eta, model_kwargs={"low_res": lr},
                                                step_noise=draws[1:], **kw)
    for o in gen:
        trace.append((float(o["sample"].mean()), float(o["pred_xstart"].mean())))
        last = o
    g = golden("sampler.npz")
    assert rel_err(last["sample"].cpu().numpy(), g[tag + "/sample"]) < 1e-3, tag
    assert np.allclose(np.array(trace), g[tag + "/trace"], rtol=1e-3, atol=1e-4)


def test_sampler_loop_f16x3_vs_reference_golden(golden):
    """BASELINE config 1 end to end with the 3x3x3 convs in split-f16 mode: same 1e-3 bar."""
    model, diff = build(TINY, "10", precision="f16x3")
    shape = (1, 1, 32, 32, 32)
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 11, seed=10)]
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).cuda()
    out = diff.p_sample_loop(model, shape, draws[0], model_kwargs={"low_res": lr}, step_noise=draws[1:])
    assert rel_err(out.cpu().numpy(), golden("sampler.npz")["ddpm10_32/sample"]) < 1e-3


def _residual_stream_io(plan):
    """io_dtype of every conv step of a plan that writes the residual stream: an NDHWC tensor that convs read (the
    tiny network has no attention, so that is every conv but the last, which stores the NCDHW output)"""
    import guided_diffusion._hip as H
    convs = [a[0]._obj for fn, a in plan.steps if fn.__name__ in ("ddpm3d_conv3d", "ddpm3d_conv3d_skip")]
    assert convs[-1].out_layout == H.OUT_NCDHW and not convs[-1].io_dtype & H.IO_OUT_BF16
    return [d.io_dtype for d in convs[:-1]]


def test_convert_to_fp16_ddim_psnr(golden):
    """BASELINE config 4 shape of run (DDIM respaced sampler, half-precision conv operands) on the
    tiny net: model.convert_to_fp16() as scripts/test.py:33-34 calls it.  Judged by PSNR against
    the fp32 reference output, not by the fp32 parity bar."""
    model, diff = build(TINY, "ddim10")
    model.convert_to_fp16()
    assert model.dtype == torch.float16 and model.conv_precision == "f16"
    shape = (2, 1, 8, 16, 16)
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 11, seed=10)]
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).cuda()
    out = diff.ddim_sample_loop(model, shape, draws[0], model_kwargs={"low_res": lr}, step_noise=draws[1:])
    ref = golden("sampler.npz")["ddim10_8x16x16/sample"]
    mse = float(((out.cpu().numpy() - ref) ** 2).mean())
    psnr = 10 * np.log10(4.0 / mse)            # data range [-1, 1]
    assert psnr > 35.0, psnr
    # the torso's tensors are STORED in f16 too, as the reference's --use_fp16 does (unet.py:1035)
    import guided_diffusion._hip as H
    plan = model.engine().plan(*[shape[0]] + list(shape[2:]))
    stream = _residual_stream_io(plan)
    assert plan.half_dtype == torch.float16 and stream
    assert all(io & H.IO_OUT_BF16 and io & H.IO_HALF_IS_F16 for io in stream)
    # (the f16x3 plan of the same network stores nothing in 16 bits)
    plain = build(TINY)[0]
    stream32 = _residual_stream_io(plain.engine().plan(*[shape[0]] + list(shape[2:])))
    assert stream32 and not any(io & (H.IO_OUT_BF16 | H.IO_HALF_IS_F16) for io in stream32)
    assert set(model.state_dict()) == set(plain.state_dict())   # parameters stay fp32 / same keys
    assert all(v.dtype == torch.float32 for v in model.state_dict().values())


def test_bf16_mode_ddim_psnr(golden):
    """BASELINE config 4's arithmetic on the tiny net: model.convert_to_bf16() -- bf16 operands on the
    matrix cores AND the residual stream stored in bf16 (fp32 statistics, timestep path, network input
    and output).  Judged by PSNR against the fp32 REFERENCE output like the fp16 mode;
    bf16 carries 8 significant bits against f16's 11, so the bar sits ~18 dB lower."""
    model, diff = build(TINY, "ddim10")
    model.convert_to_bf16()
    assert model.dtype == torch.bfloat16 and model.conv_precision == "bf16"
    shape = (2, 1, 8, 16, 16)
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 11, seed=10)]
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).cuda()
    out = diff.ddim_sample_loop(model, shape, draws[0], model_kwargs={"low_res": lr}, step_noise=draws[1:])
    assert out.dtype == torch.float32 and torch.isfinite(out).all()
    ref = golden("sampler.npz")["ddim10_8x16x16/sample"]
    mse = float(((out.cpu().numpy() - ref) ** 2).mean())
    psnr = 10 * np.log10(4.0 / mse)            # data range [-1, 1]
    print("bf16 mode, tiny net, ddim10: PSNR vs the reference's fp32 output %.1f dB" % psnr)
    assert psnr > 30.0, psnr            # measured 35.7 dB
    assert all(v.dtype == torch.float32 for v in model.state_dict().values())
    # the plan really stores the residual stream in bf16
    import guided_diffusion._hip as H
    plan = next(iter(model.engine().plans.values()))
    stream = _residual_stream_io(plan)
    assert plan.half_dtype == torch.bfloat16 and stream
    assert all(io & H.IO_OUT_BF16 and not io & H.IO_HALF_IS_F16 for io in stream)


def test_p_sample_loop_api_and_determinism():
    """Positional noise argument as scripts/test.py:63-69 passes it; result shape/dtype/device;
    bitwise repeatability with injected noise (no atomics anywhere in the path)."""
    model, diff = build(TINY, "10")
    shape = (1, 1, 8, 16, 16)
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 11, seed=10)]
    lr = torch.from_numpy(synth.synth_low_res(shape, seed=1234)).cuda()
    a = diff.p_sample_loop(model, shape, draws[0], clip_denoised=True, model_kwargs={"low_res": lr},
                           step_noise=draws[1:])
    b = diff.p_sample_loop(model, shape, draws[0], clip_denoised=True, model_kwargs={"low_res": lr},
                           step_noise=draws[1:])
    assert a.shape == shape and a.dtype == torch.float32 and a.is_cuda
    assert torch.equal(a, b)
    c = diff.p_sample_loop(model, shape, model_kwargs={"low_res": lr})  # device RNG path
    assert torch.isfinite(c).all()


def test_full_size_forward_properties():
    """BASELINE config 2's forward at FULL size (published architecture, 1 x 64^3, 5 831 GFLOP) --
    too large for the CPU oracle inside a test, so it is held to size-independent properties:
      (1) the default path (f16x3 arithmetic, Winograd-D kernels incl. the wave-specialised one that
          only the 64^3 level selects, split-K, weight-stationary order) agrees with the exact
          fp32-MFMA mode -- itself pinned to the reference at reduced sizes above -- within the
          single-forward bar;
      (2) two runs are bit-identical (no atomics, no data-dependent scheduling);
      (3) a volume's result does not depend on what else is in its batch (different tile counts
          change the split-K factors, i.e. summation orders: rounding-level differences only)."""
    shape = (1, 1, 64, 64, 64)
    x, lr = inputs(shape)
    x2 = torch.from_numpy(synth.synth_noise(shape, 1, seed=4)[0])
    lr2 = torch.from_numpy(synth.synth_low_res(shape, seed=99))
    t = torch.tensor([617])
    model, _ = build(PUBLISHED)                       # default precision
    assert model.conv_precision == "f16x3"
    with torch.no_grad():
        y = model(x.cuda(), t.cuda(), low_res=lr.cuda())
        y_again = model(x.cuda(), t.cuda(), low_res=lr.cuda())
        yb = model(torch.cat([x, x2]).cuda(), torch.tensor([617, 41]).cuda(), low_res=torch.cat([lr, lr2]).cuda())
    assert tuple(y.shape) == (1, 2, 64, 64, 64) and torch.isfinite(y).all()
    assert torch.equal(y, y_again)
    assert rel_err(yb[0:1].cpu().numpy(), y.cpu().numpy()) < 2e-5
    y_def = y.cpu().numpy()
    del model, y, y_again, yb
    torch.cuda.empty_cache()
    exact, _ = build(PUBLISHED, precision="f32")
    with torch.no_grad():
        y_exact = exact(x.cuda(), t.cuda(), low_res=lr.cuda()).cpu().numpy()
    assert rel_err(y_def, y_exact) < 1e-4


def test_full_size_forward_vs_cpu_oracle():
    """full-size parity must not rest on self-comparison.  ONE published-architecture
    forward at BASELINE config 2's size (1 x 64^3; 5 831 GFLOP, a few seconds of host time) through the
    CPU oracle -- which is pinned to the reference's own outputs (tests/test_oracle_golden.py) --
    against the GPU in BOTH arithmetics, per output channel (the eps and the variance channel each on
    its own scale) at the single-forward bar.  Covers what only appears above 32-wide grids: second
    z-tile rows, XCD orders with > 2048 workgroups, offsets beyond 2^31 bits."""
    from oracle import unet_ref
    shape = (1, 1, 64, 64, 64)
    x, lr = inputs(shape)
    t = torch.tensor([617])
    model, _ = build(PUBLISHED)
    assert model.conv_precision == "f16x3"
    cfg = unet_ref.sr_config(**PUBLISHED)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    torch.set_num_threads(min(16, torch.get_num_threads() or 16))
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, cfg, x, t, lr).numpy()
        y = model(x.cuda(), t.cuda(), low_res=lr.cuda()).cpu().numpy()
    assert rel_err_per_channel(y, ref) < 1e-4
    del model
    torch.cuda.empty_cache()
    exact, _ = build(PUBLISHED, precision="f32")
    with torch.no_grad():
        y32 = exact(x.cuda(), t.cuda(), low_res=lr.cuda()).cpu().numpy()
    assert rel_err_per_channel(y32, ref) < 1e-4


def test_batch_beyond_32bit_addressing_is_split():
    """One launch addresses a tensor with 32-bit byte offsets (the C ABI refuses more: "split the
    batch").  The engine does the splitting: 130 volumes of 64^3 through the tiny net make 4.4 GB
    full-resolution activations; the forward runs as halves and every volume equals its own
    batch-1 result."""
    model, _ = build(TINY)
    N = 130
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 1, 64, 64, 64, generator=g)
    lr = torch.rand(N, 1, 64, 64, 64, generator=g)
    t = torch.randint(0, 1000, (N,), generator=g)
    with torch.no_grad():
        y = model(x.cuda(), t.cuda(), low_res=lr.cuda())
        assert tuple(y.shape) == (N, 2, 64, 64, 64) and torch.isfinite(y).all()
        eng = model.engine()
        assert eng.split_above[(64, 64, 64)] < N          # the refusal was met and handled
        for n in (0, 64, 65, 129):
            y1 = model(x[n:n + 1].cuda(), t[n:n + 1].cuda(), low_res=lr[n:n + 1].cuda())
            assert rel_err(y[n:n + 1].cpu().numpy(), y1.cpu().numpy()) < 2e-5, n
    del y
    torch.cuda.empty_cache()


def test_cpu_tensors_are_refused():
    model, diff = build(TINY, "10")
    x, lr = inputs((1, 1, 4, 16, 16))
    with pytest.raises(RuntimeError, match="GPU"):
        model(x, torch.tensor([1]), low_res=lr)


# ---------------------------------------------------------------- the 2-D network (create_model)
MODEL2D_VARIANTS = {
    "film": {},
    "updown_additive": dict(resblock_updown=True, use_scale_shift_norm=False, learn_sigma=False),
}


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("tag", sorted(MODEL2D_VARIANTS))
def test_model2d_forward_and_loops_vs_reference_golden(golden, tag, precision):
    """create_model_and_diffusion (script_util.py:74-184): the 2-D RGB UNetModel (dims=2, 3 channels
    in, 3 or 6 out, attention at ds 4 and in the middle block, strided-conv or ResBlock resampling)
    on the HIP engine -- (N, 3, H, W) images run as depth-1 volumes -- against the reference's own
    forward and 6-step DDPM / DDIM loops (tests/golden/model2d.npz)."""
    fl = su.model_and_diffusion_defaults()
    fl.update(image_size=64, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", num_head_channels=32,
              attention_resolutions="16", learn_sigma=True, use_scale_shift_norm=True, timestep_respacing="6")
    fl.update(MODEL2D_VARIANTS[tag])
    model, diff = su.create_model_and_diffusion(**fl)
    model.conv_precision = precision
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape), 2))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    g = golden("model2d.npz")
    shape = (2, 3, 32, 48)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=3)[0]).cuda()
    with torch.no_grad():
        y = model(x, torch.tensor([617, 3]).cuda())
    assert tuple(y.shape) == g[tag + "/forward"].shape
    assert rel_err_per_channel(y.cpu().numpy(), g[tag + "/forward"]) < 2e-5
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 7, seed=10)]
    a = diff.p_sample_loop(model, shape, draws[0], step_noise=draws[1:])
    b = diff.ddim_sample_loop(model, shape, draws[0], step_noise=draws[1:])
    ea, eb = rel_err(a.cpu().numpy(), g[tag + "/ddpm"]), rel_err(b.cpu().numpy(), g[tag + "/ddim"])
    print("2-D %s %s: ddpm %.2e ddim %.2e" % (tag, precision, ea, eb))
    assert ea < 1e-3 and eb < 1e-3              # the north_star bar, as for the 3-D loops above
    with pytest.raises(RuntimeError):
        model(x.unsqueeze(2), torch.tensor([617, 3]).cuda())      # a dims=2 model takes 4-D tensors


# ---------------------------------------------------------------- class conditioning, new attention order
def test_class_conditional_sr_model_vs_reference_golden(golden):
    """class_cond=True through sr_create_model_and_diffusion (script_util.py:442: label_emb of 1000
    classes, unet.py:476-478, :703-705): forward with y and a 3-step p_sample_loop with y in
    model_kwargs, against the reference's outputs; a missing / out-of-range y fails like the reference."""
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(TINY, class_cond=True, timestep_respacing="3")
    model, diff = su.sr_create_model_and_diffusion(**fl)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape), 4))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    g = golden("api_extras.npz")
    shape = (2, 1, 4, 16, 16)
    x, lr = inputs(shape)
    y = torch.from_numpy(g["sr_class_cond/y"]).cuda()
    with torch.no_grad():
        out = model(x.cuda(), torch.tensor([37, 999]).cuda(), low_res=lr.cuda(), y=y)
    assert rel_err_per_channel(out.cpu().numpy(), g["sr_class_cond/forward"]) < 1e-4
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 4, seed=10)]
    a = diff.p_sample_loop(model, shape, draws[0], model_kwargs={"low_res": lr.cuda(), "y": y}, step_noise=draws[1:])
    assert rel_err(a.cpu().numpy(), g["sr_class_cond/ddpm3"]) < 1e-3
    with pytest.raises(AssertionError):
        model(x.cuda(), torch.tensor([37, 999]).cuda(), low_res=lr.cuda())
    with pytest.raises(IndexError):
        model(x.cuda(), torch.tensor([37, 999]).cuda(), low_res=lr.cuda(), y=torch.tensor([0, 1000]).cuda())


@pytest.mark.parametrize("tag,over", [
    ("new_order", dict(use_new_attention_order=True)),
    ("new_order_class_cond", dict(use_new_attention_order=True, class_cond=True, num_head_channels=-1, num_heads=2)),
])
def test_new_attention_order_vs_reference_golden(golden, tag, over):
    """use_new_attention_order=True (QKVAttention, unet.py:361-389) through create_model_and_diffusion: the
    qkv conv's output channels are permuted at pack time and the same attention kernel runs; forward
    and a 6-step loop against the reference (with class conditioning in the second variant)."""
    fl = su.model_and_diffusion_defaults()
    fl.update(image_size=64, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", num_head_channels=32,
              attention_resolutions="16", learn_sigma=True, use_scale_shift_norm=True, timestep_respacing="6")
    fl.update(over)
    model, diff = su.create_model_and_diffusion(**fl)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape), 2))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    g = golden("api_extras.npz")
    shape = (2, 3, 32, 48)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=3)[0]).cuda()
    kw = {"y": torch.tensor([5, 0]).cuda()} if over.get("class_cond") else {}
    with torch.no_grad():
        out = model(x, torch.tensor([617, 3]).cuda(), **kw)
    assert rel_err_per_channel(out.cpu().numpy(), g[tag + "/forward"]) < 2e-5
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 7, seed=10)]
    a = diff.p_sample_loop(model, shape, draws[0], model_kwargs=kw, step_noise=draws[1:])
    assert rel_err(a.cpu().numpy(), g[tag + "/ddpm"]) < 1e-3


def test_superres_model_with_several_image_channels():
    """A SuperRes model built directly with in_channels != 1 (the reference's RGB super-resolution
    networks): the two-pointer planar first conv is for one image + one low_res channel
    only, so such a model concatenates at the edge (unet.py:1693) -- and must equal the oracle."""
    from guided_diffusion.unet import SuperResModel_noatt
    from oracle import unet_ref
    model = SuperResModel_noatt(96, 3, 32, 6, 1, (), channel_mult=(1, 2), dims=3, num_head_channels=32,
                                use_scale_shift_norm=True, resblock_updown=True)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape), 6))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    shape = (1, 3, 4, 16, 16)
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=3)[0])
    lr = torch.from_numpy(synth.synth_noise(shape, 1, seed=5)[0])
    with torch.no_grad():
        out = model(x.cuda(), torch.tensor([11]).cuda(), low_res=lr.cuda())
    cfg = dict(in_channels=6, model_channels=32, out_channels=6, num_res_blocks=1, attention_ds=(), channel_mult=(1, 2),
               num_heads=1, num_head_channels=32, num_heads_upsample=1, use_scale_shift_norm=True,
               resblock_updown=True, mid_attention=False)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, cfg, x, torch.tensor([11]), lr)
    assert rel_err_per_channel(out.cpu().numpy(), ref.numpy()) < 1e-4
    with pytest.raises(RuntimeError):
        model(x.cuda(), torch.tensor([11]).cuda(), low_res=lr[:, :, :2].cuda())


def test_step_graph_replay_equals_eager_launches():
    """the forward as ONE captured hipGraph (engine.py: _Plan._replay) against the same plan
    issued launch by launch -- same kernels, same arguments: bitwise equal.  Covers the sampler's fast path
    (one film row shared by the batch, the step's x and row copied into the captured buffers), the module
    call with one timestep per sample (a film row per sample), a second conditioning volume through the same
    graph, and a whole 10-step loop."""
    model, diff = build(TINY, "10")
    shape = (2, 1, 8, 16, 16)
    x, lr = inputs(shape)
    lr2 = torch.from_numpy(synth.synth_low_res(shape, seed=99))
    t = torch.tensor([37, 999])
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 11, seed=10)]
    res = {}
    for graph in (False, True):
        model.step_graph = graph
        with torch.no_grad():
            y = model(x.cuda(), t.cuda(), low_res=lr.cuda())
            y2 = model(x.cuda(), t.cuda(), low_res=lr2.cuda())
            y3 = model(x.cuda(), t.cuda(), low_res=lr.cuda())
            s = diff.p_sample_loop(model, shape, draws[0], model_kwargs={"low_res": lr.cuda()}, step_noise=draws[1:])
        res[graph] = (y.cpu(), y2.cpu(), y3.cpu(), s.cpu())
    eng = model.engine()
    assert eng.step_graph and any(pl.graphs for pl in eng.plans.values())      # the graph path really ran
    for a, b in zip(res[False], res[True]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(res[True][0], res[True][2]) and not torch.equal(res[True][0], res[True][1])


@pytest.mark.parametrize("tag,over,shape,t,precision", [
    ("tiny", {}, (2, 1, 8, 16, 16), [37, 999], "f16x3"),
    ("tiny exact", {}, (1, 1, 5, 48, 16), [3], "f32"),
    ("tiny additive", dict(use_scale_shift_norm=False), (1, 1, 4, 16, 16), [5], "f16x3"),
    ("tiny conv resample", dict(resblock_updown=False), (1, 1, 4, 16, 16), [5], "f16x3"),
    ("tiny attention", dict(large_size=32, attention_resolutions="8,4", num_head_channels=32), (1, 1, 8, 32, 32), [10], "f16x3"),
    ("tiny bf16", {}, (1, 1, 8, 16, 16), [500], "bf16"),
    ("tiny f16", {}, (1, 1, 8, 16, 16), [500], "f16"),
    ("published", None, (1, 1, 8, 32, 32), [251], "f16x3"),
    # (the one-MFMA modes run the lean epilogue in their Winograd kernels, split levels and 4x4x8 tiles included)
    ("published bf16", None, (1, 1, 8, 32, 32), [251], "bf16"),
    ("published f16", None, (1, 1, 8, 32, 32), [251], "f16"),
])
def test_native_plan_equals_python_plan(tag, over, shape, t, precision):
    """The planner and its two replayers: the whole-network level of the C ABI (ddpm3d_unet_plan_create /
    ddpm3d_unet_forward: libddpm3d compiles the launch list into one caller-provided arena and replays it -- SURVEY
    8b's `unet_forward(handle, ...)`) against the Python host's launch-by-launch replay of the list of the same
    model: the same per-op calls in the same order, so the outputs are BITWISE
    equal, per architecture variant and arithmetic; also through the sampler's fast path (one film row shared
    by the batch), with the step graph on top, and for a second shape of the same model."""
    model, diff = build(PUBLISHED if over is None else dict(TINY, **over), "10", precision=precision)
    x, lr = inputs(shape)
    tt = torch.tensor(t[:shape[0]])
    res = {}
    for native in (False, True):
        model.native_plan = native
        with torch.no_grad():
            y = model(x.cuda(), tt.cuda(), low_res=lr.cuda())
            draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 4, seed=10)]
            it = diff.p_sample_loop_progressive(model, shape, draws[0], model_kwargs={"low_res": lr.cuda()},
                                                step_noise=draws[1:] + draws[1:] * 4)
            s = [next(it)["sample"].clone() for _ in range(3)]
        res[native] = [y.cpu()] + [v.cpu() for v in s]
    eng = model.engine()
    assert eng.native_plan and eng.native_plans                      # the C-level plan really ran
    for a, b in zip(res[False], res[True]):
        assert torch.isfinite(a).all() and torch.equal(a, b), tag
    # a captured graph of the C-level forward, and another shape through the same description
    model.step_graph = True
    with torch.no_grad():
        yg = model(x.cuda(), tt.cuda(), low_res=lr.cuda())
    assert torch.equal(yg.cpu(), res[True][0])
    model.step_graph = False
    shape2 = (1, 1, 4, 16, 16)
    x2, lr2 = inputs(shape2)
    with torch.no_grad():
        a = model(x2.cuda(), tt[:1].cuda(), low_res=lr2.cuda())
        model.native_plan = False
        b = model(x2.cuda(), tt[:1].cuda(), low_res=lr2.cuda())
    assert torch.equal(a, b)


def test_native_plan_runs_the_2d_network_and_refuses_bad_arenas():
    """create_model_and_diffusion's 2-D RGB network (ordinary multi-channel input, padded at the edge) through the
    library's replay, bitwise equal to the Python replay; and the C entry points refuse a NULL / undersized arena."""
    import ctypes as C
    import guided_diffusion._hip as H
    from guided_diffusion import script_util as su
    fl = su.model_and_diffusion_defaults()
    fl.update(image_size=64, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", num_head_channels=32,
              attention_resolutions="16", learn_sigma=True, use_scale_shift_norm=True, timestep_respacing="6")
    model, _ = su.create_model_and_diffusion(**fl)
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape))) for k, v in sd.items()})
    model.to("cuda").eval()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 32, 48, generator=g).cuda()
    t = torch.tensor([5, 700]).cuda()
    with torch.no_grad():
        a = model(x, t)
        model.native_plan = True
        b = model(x, t)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    eng = model.engine()
    lib, desc = eng.lib, eng.native_desc()
    need = lib.ddpm3d_unet_plan_bytes(C.byref(desc), 1, 1, 32, 48)
    assert need > 0
    handle = C.c_void_p()
    small = torch.empty(need // 2, dtype=torch.uint8, device="cuda")
    assert lib.ddpm3d_unet_plan_create(C.byref(desc), 1, 1, 32, 48, H.ptr(small), need // 2, C.byref(handle)) == H.E_INVAL
    assert b"the plan needs" in lib.ddpm3d_unet_last_error()
    assert lib.ddpm3d_unet_plan_create(C.byref(desc), 1, 1, 32, 48, 0, need, C.byref(handle)) == H.E_INVAL
    assert lib.ddpm3d_unet_plan_bytes(C.byref(desc), 0, 1, 32, 48) == 0


# ---------------------------------------------------------------- step noise of the wrong shape
# The step kernels read one noise draw per element of x, so a noise tensor of another shape is refused before the
# step launches.  The tensors here are oversized: a kernel that took one would still read only inside it.
def _oversized(shape):
    return torch.zeros((shape[0] + 1,) + tuple(shape[1:]), device="cuda")


@pytest.mark.parametrize("loop", ["p_sample", "ddim_sample", "dpm_solver_sde", "calc_bpd"])
def test_loop_step_noise_of_wrong_shape_is_refused(loop):
    model, diff = build(TINY, "2")
    shape = (1, 1, 4, 16, 16)
    x, lr = inputs(shape)
    kw = {"low_res": lr.cuda()}
    bad = [_oversized(shape)] * diff.num_timesteps
    with pytest.raises(AssertionError):
        if loop == "calc_bpd":
            diff.calc_bpd_loop(model, x.cuda(), model_kwargs=kw, step_noise=bad)
        elif loop == "dpm_solver_sde":
            next(diff.dpm_solver_sample_loop_progressive(model, shape, x.cuda(), model_kwargs=kw, order=1,
                                                         stochastic=True, step_noise=bad))
        else:
            next(getattr(diff, loop + "_loop_progressive")(model, shape, x.cuda(), model_kwargs=kw, step_noise=bad))


@pytest.mark.parametrize("step", ["p_sample", "ddim_sample"])
def test_step_noise_of_wrong_shape_is_refused(step):
    model, diff = build(TINY, "2")
    shape = (1, 1, 4, 16, 16)
    x, lr = inputs(shape)
    with pytest.raises(AssertionError):
        getattr(diff, step)(model, x.cuda(), torch.tensor([1]).cuda(), model_kwargs={"low_res": lr.cuda()},
                            noise=_oversized(shape))
