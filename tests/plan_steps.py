"""
What the plan-step goldens (tests/golden/plan_steps.json) are made of, shared by their generator
(tests/golden/make_plan_steps.py), the CPU test of the planner and the GPU test of the two replayers: the cases, the
models, the signature of a step list, and the forward / sampler-step outputs whose bits are pinned.
"""

import contextlib
import ctypes as C
import hashlib
import json
import os
import types

import torch

import guided_diffusion._hip as H
from guided_diffusion import engine as E
from guided_diffusion import script_util as su
from guided_diffusion import synth

PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)
MODEL2D = dict(image_size=64, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", num_head_channels=32,
               attention_resolutions="16", learn_sigma=True, use_scale_shift_norm=True)

Case = types.SimpleNamespace
# name -> flags over TINY (None: the published network; "2d": the 2-D RGB network), input shape, timesteps, arithmetic,
# engine switches set through the environment
CASES = {
    "tiny": Case(over={}, shape=(2, 1, 8, 16, 16), t=[37, 999], precision="f16x3", env={}),
    "tiny exact": Case(over={}, shape=(1, 1, 5, 48, 16), t=[3], precision="f32", env={}),
    "tiny additive": Case(over=dict(use_scale_shift_norm=False), shape=(1, 1, 4, 16, 16), t=[5], precision="f16x3", env={}),
    "tiny conv resample": Case(over=dict(resblock_updown=False), shape=(1, 1, 4, 16, 16), t=[5], precision="f16x3", env={}),
    "tiny attention": Case(over=dict(large_size=32, attention_resolutions="8,4", num_head_channels=32),
                           shape=(1, 1, 8, 32, 32), t=[10], precision="f16x3", env={}),
    "tiny bf16": Case(over={}, shape=(1, 1, 8, 16, 16), t=[500], precision="bf16", env={}),
    "tiny f16": Case(over={}, shape=(1, 1, 8, 16, 16), t=[500], precision="f16", env={}),
    "published": Case(over=None, shape=(1, 1, 8, 32, 32), t=[251], precision="f16x3", env={}),
    "published bf16": Case(over=None, shape=(1, 1, 8, 32, 32), t=[251], precision="bf16", env={}),
    "published f16": Case(over=None, shape=(1, 1, 8, 32, 32), t=[251], precision="f16", env={}),
    "model2d": Case(over="2d", shape=(2, 3, 32, 48), t=[5, 700], precision="f16x3", env={}),
    "published two-call skips": Case(over=None, shape=(1, 1, 8, 32, 32), t=[251], precision="f16x3",
                                     env={"DDPM3D_SKIP_FUSE": "0"}),
    "published 36-tap up convs": Case(over=None, shape=(1, 1, 8, 32, 32), t=[251], precision="f16x3",
                                      env={"DDPM3D_UP_PHASE": "0"}),
}


# the cases whose step lists are committed in full (tests/golden/plan_steps_small.json; the others as digests: all
# thirteen lists are a quarter of a megabyte): between them every kind of step and every per-call role
SMALL = ("tiny additive", "model2d")


@contextlib.contextmanager
def switches(case):
    """the engine reads its switches from the environment when it is built"""
    names = ("DDPM3D_SKIP_FUSE", "DDPM3D_UP_PHASE")
    keep = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(case.env)
    try:
        yield
    finally:
        for k in names:
            os.environ.pop(k, None)
            if keep[k] is not None:
                os.environ[k] = keep[k]


def build(case, device=None):
    """(model, diffusion) of a case; with a device, the synthetic parameters on it"""
    if case.over == "2d":
        fl = su.model_and_diffusion_defaults()
        fl.update(MODEL2D, timestep_respacing="6")
        model, diff = su.create_model_and_diffusion(**fl)
    else:
        fl = su.sr_model_and_diffusion_defaults()
        fl.update(PUBLISHED if case.over is None else dict(TINY, **case.over), timestep_respacing="10")
        model, diff = su.sr_create_model_and_diffusion(**fl)
    model.conv_precision = case.precision
    if device is not None:
        model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape)))
                               for k, v in model.state_dict().items()})
        model.to(device).eval()
    return model, diff


# ---------------------------------------------------------------- the signature of a step list
def _struct(s, named, pid):
    vals = []
    for field, typ in s._fields_:
        v = getattr(s, field)
        if field in named:
            vals.append(named[field])
        elif field == "workspace":
            vals.append(bool(v))                # attached or not: one buffer shared by the plan
        elif typ is C.c_void_p:
            vals.append(pid(v))
        else:
            vals.append(v)
    return vals


def signature(plan, planar):
    """Per step: the entry's name and every argument that is not a pointer (for convs: every scalar field of the
    descriptor), with each pointer replaced by "p<index of its first appearance in the list>" (NULL stays None) and the
    pointers of the forward call by their names.  Pins the dataflow and the buffer reuse, not the addresses."""
    ids = {}

    def pid(v):
        return None if not v else "p%d" % ids.setdefault(v, len(ids))

    first = C.addressof(plan.first_desc) if planar and plan.first_desc is not None else None
    last = C.addressof(plan.last_desc)
    bias = {C.addressof(d): off for d, off in plan.bias_patches}
    film = {id(a) for a in plan.film_patches}
    out = []
    for fn, args in plan.steps:
        name, vals = fn.__name__, []
        if name in ("ddpm3d_conv3d", "ddpm3d_conv3d_skip"):
            d = args[0]._obj
            a, named = C.addressof(d), {}
            if a == first:
                named.update(src0="x", src1="low_res")
            if a == last:
                named.update(out="out")
            if a in bias:
                named.update(bias="film+%d" % bias[a], bias_stride_n="film_stride")
            vals.append(_struct(d, named, pid))
            if name == "ddpm3d_conv3d_skip":
                vals.append(_struct(args[1]._obj, {}, pid))
        else:
            named = {}
            if args is plan.absmax_args:
                named = {0: "x", 1: "low_res" if planar else None}
            elif args is getattr(plan, "pad_args", None):
                named = {0: "x"}
            elif id(args) in film:
                named = {12: "film", 13: "film_stride"}
            for k, (typ, v) in enumerate(zip(H.EXPORTS[name][1][:-1], args[:-1])):     # (the last slot is the stream)
                if k in named:
                    vals.append(named[k])
                elif typ is C.c_void_p:
                    vals.append(pid(v))
                elif typ is C.c_float:
                    vals.append(C.c_float(v).value)
                else:
                    vals.append(v)
        out.append([name, vals])
    return out


def meta(plan):
    """conv_meta as [[step index, tag, FLOPs]]"""
    return [[i, tag, fl] for i, (tag, fl) in sorted(plan.conv_meta.items())]


ENTRY_LETTER = {"ddpm3d_conv3d": "c", "ddpm3d_conv3d_skip": "s", "ddpm3d_gn_finalize": "f", "ddpm3d_absmax": "a",
                "ddpm3d_ncdhw_to_ndhwc_pad": "n", "ddpm3d_pool_act": "p", "ddpm3d_attention_p": "t"}


def digest(sig, conv_meta):
    """What the golden keeps of a signature and a conv_meta list: the sha256 of each (of its compact JSON text: equal
    digests = equal lists, every scalar and every pointer index), and, to make a difference readable, the entry of every
    step as one letter and per kernel family the launches and their FLOPs."""
    def sha(v):
        return hashlib.sha256(json.dumps(v, separators=(",", ":")).encode()).hexdigest()

    families = {}
    for _, tag, fl in conv_meta:
        f = families.setdefault(tag, [0, 0.0])
        f[0], f[1] = f[0] + 1, f[1] + fl
    return {"entries": "".join(ENTRY_LETTER[name] for name, _ in sig), "steps_sha256": sha(sig),
            "conv_meta_sha256": sha(conv_meta), "families": dict(sorted(families.items()))}


def ndhw(shape):
    """a plan's key from an input shape (a 2-D image runs as a depth-1 volume)"""
    return (shape[0], 1) + tuple(shape[2:]) if len(shape) == 4 else (shape[0],) + tuple(shape[2:])


def planner_steps(lib, desc, shape, arena):
    """Size and create a C plan on `arena` (an address; never dereferenced by the planner) and translate its steps:
    (the handle -- the translated steps point into it --, the arena's size, the replay list as a namespace)"""
    N, D, Hh, W = ndhw(shape)
    need = lib.ddpm3d_unet_plan_bytes(C.byref(desc), N, D, Hh, W)
    if need == 0:
        raise RuntimeError(lib.ddpm3d_unet_last_error().decode())
    handle = C.c_void_p()
    rc = lib.ddpm3d_unet_plan_create(C.byref(desc), N, D, Hh, W, arena, need, C.byref(handle))
    if rc != 0:
        raise H.Ddpm3dError(rc, lib.ddpm3d_unet_last_error().decode())
    return handle, need, E.replay_list(lib, E.plan_records(lib, handle))


def fake_addresses():
    """name -> a 256-byte aligned address that stands for that tensor (the planner only stores it)"""
    table = {}
    return lambda name: table.setdefault(name, (1 << 40) + 256 * len(table))


def host_desc(model, addr):
    """the description of a model that has no engine (no device): topology and parameter shapes only"""
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    a = model.engine_args()
    cin_pad = (a["in_channels"] + 15) // 16 * 16
    conv = E.conv_shapes(shapes, model.topology.input[0][0].prefix, None if a["planar"] else cin_pad)
    up_phase, skip_fuse = E.switches(model.conv_precision, a["winograd"])
    return E.unet_desc(model.topology, conv, E.film_offsets(model.topology, shapes)[0], addr, model.conv_precision,
                       model.use_scale_shift_norm, a["planar"], a["in_channels"], cin_pad, a["winograd"], up_phase,
                       skip_fuse)


# ---------------------------------------------------------------- the outputs whose bits are pinned
def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def outputs(model, diff, case):
    """sha256 of one forward and of the first three steps of a p_sample_loop on fixed inputs"""
    shape = case.shape
    x = torch.from_numpy(synth.synth_noise(shape, 1, seed=3)[0]).cuda()
    kw = {} if case.over == "2d" else {"low_res": torch.from_numpy(synth.synth_low_res(shape, seed=1234)).cuda()}
    with torch.no_grad():
        y = model(x, torch.tensor(case.t[:shape[0]]).cuda(), **kw)
        draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(shape, 4, seed=10)]
        it = diff.p_sample_loop_progressive(model, shape, draws[0], model_kwargs=kw, step_noise=draws[1:] + draws[1:] * 4)
        steps = [next(it)["sample"].clone() for _ in range(3)]
    return [_sha(v) for v in [y] + steps]
