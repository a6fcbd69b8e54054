"""
The Python host of the 3-D UNet forward: it describes a model to the library
and replays the launch plan the library compiles.

A model (its layer list from unet.py and its parameters) plus an input shape
(N, D, H, W) is compiled ONCE, by libddpm3d (csrc/unet_plan.hip, the only
planner), into a flat list of C-ABI calls with every buffer, descriptor and
statistics row count fixed; a forward pass replays the list -- from here,
launch by launch (_Plan: the replay that can time every conv), or inside the
library (_NativePlan).  Nothing in this module decides how a layer runs.
What the reference does as ~600 ATen calls per step
(unet.py:1015-1044, :236-256) becomes, per ResBlock,

    gn_finalize -> conv3d(GN+SiLU [+pool/up] prologue, stats epilogue)
    gn_finalize(FiLM) -> [conv3d k=1 skip] -> conv3d(GN*(1+s)+t, SiLU prologue;
                                                      + residual, stats epilogue)

Activations live channels-last ([N][D][H][W][C], fp32).  The timestep path
(timestep_embedding -> time_embed -> every ResBlock's emb_layers) does not
depend on x, so all emb_layers are fused into one Linear whose output row
("film row") is either computed per call or, in the samplers, precomputed
for every step of the schedule.
"""

import collections
import ctypes as C
import math
import os
import types

import torch

from . import _hip as H


class PackedConv:
    __slots__ = ("w", "b", "Cout", "Cin", "k", "precision", "wz", "up_phase")

    def __init__(self, weight, bias, precision, stream):
        lib = H.load()
        self.wz = None   # optional Winograd-along-depth packing of the same layer
        self.up_phase = False   # w is ddpm3d_pack_up_phase_weight's image (pack_up_phase)
        Cout, Cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
        n = lib.ddpm3d_packed_weight_bytes(Cout, Cin, k, precision)
        if n == 0:
            raise RuntimeError("unsupported conv weight shape %s" % (tuple(weight.shape),))
        w32 = weight.detach().float().contiguous()
        self.w = torch.empty(n, dtype=torch.uint8, device=weight.device)
        H.check(lib.ddpm3d_pack_conv_weight(H.ptr(w32), Cout, Cin, k, precision, H.ptr(self.w), stream))
        self.b = bias.detach().float().contiguous()
        self.Cout, self.Cin, self.k, self.precision = Cout, Cin, k, precision

    def pack_up_phase(self, weight, stream):
        """Replace this f16x3 Winograd-D image by the phase image of the same weights (it starts with the same
        Winograd-D image): the layer's IN_UP calls then carry HINT_UP_PHASE."""
        lib = H.load()
        n = lib.ddpm3d_packed_up_phase_bytes(self.Cout, self.Cin)
        if n == 0:
            raise RuntimeError("no phase image for a %dx%d conv" % (self.Cout, self.Cin))
        w32 = weight.detach().float().contiguous()
        self.w = torch.empty(n, dtype=torch.uint8, device=weight.device)
        H.check(lib.ddpm3d_pack_up_phase_weight(H.ptr(w32), self.Cout, self.Cin, H.ptr(self.w), stream))
        self.up_phase = True


def conv_shapes(param_shapes, first, cin_pad):
    """base -> (Cout, Cin, k) of every conv as it is packed: a 3-D conv as it is; a 2-D 3x3 conv (dims=2 models) as the
    3x3x3 conv whose only non-zero depth tap is the centre one, on depth-1 volumes; Conv1d / 1x1 Conv2d pointwise.
    `first` is padded to cin_pad input channels (None: the planar first conv, as it is)."""
    out = {}
    for name, s in param_shapes.items():
        if name.endswith(".weight") and len(s) >= 3:
            base = name[:-len(".weight")]
            k = s[2] if len(s) == 5 else 3 if (len(s) == 4 and s[2] == 3) else 1
            out[base] = (s[0], cin_pad if (base == first and cin_pad) else s[1], k)
    return out


def film_offsets(topo, param_shapes):
    """(ResBlock prefix -> offset of its emb_layers output inside a film row, row length)"""
    offs, off = {}, 0
    for e in topo.all_layers():
        if e.kind == "res":
            offs[e.prefix] = off
            off += param_shapes[e.prefix + ".emb_layers.1.weight"][0]
    return offs, off


def switches(precision, winograd):
    """(up_phase, skip_fuse), the A/B switches an engine reads from the environment when it is built: DDPM3D_UP_PHASE=0
    packs no phase image (f16x3 up-ResBlocks stay on the 36-tap path), DDPM3D_SKIP_FUSE=0 keeps ResBlock tails as two steps"""
    return (bool(winograd and precision == "f16x3" and os.environ.get("DDPM3D_UP_PHASE", "1") != "0"),
            os.environ.get("DDPM3D_SKIP_FUSE", "1") != "0")


def winograd_images(topo, shapes, precision, winograd, up_phase):
    """base -> (precision of the layer's Winograd-along-depth image or None, whether that image is the phase image).
    f16x3 / f16 / bf16: the big 3x3x3 layers also get the Winograd-D form (same arithmetic, 2/3 of the MFMAs; the
    library's planner picks it per call where the shape / input mode allow); with `up_phase`, conv1 of the
    up-ResBlocks, which reads a nearest-up-sampled input, gets the phase image (four 2x2 phase convs on the
    low-resolution input, 16 taps instead of 36)."""
    prec = H.PRECISIONS[precision]
    up_conv1 = {e.prefix + ".in_layers.2" for e in topo.all_layers() if e.kind == "res" and e.updown == "up"}
    out = {}
    for base, (Cout, Cin, k) in shapes.items():
        wz = prec in H.WINOGRAD_OF and winograd and k == 3 and Cout % 128 == 0 and Cin % 16 == 0
        out[base] = (H.WINOGRAD_OF[prec] if wz else None, bool(wz and up_phase and base in up_conv1))
    return out


def unet_desc(topo, shapes, film_off, addr, precision, film, planar, in_channels, cin_pad, winograd=True, up_phase=True,
              skip_fuse=True):
    """struct ddpm3d_unet_desc of a model, from its topology, its conv shapes (conv_shapes) and the engine's switches.
    addr(name) gives the device address of a parameter (its state_dict name) or of a conv's "<base>:packed",
    "<base>:packed_wz" and "<base>:bias".  Returns (desc, the ctypes arrays it points into)."""
    images = winograd_images(topo, shapes, precision, winograd, up_phase)

    def weights(base, skip=False):
        w = H.ConvWeights()
        if base in shapes:
            w.w_packed, w.bias = addr(base + ":packed"), addr(base + ":bias")
            (w.Cout, w.Cin, w.ksize), w.precision = shapes[base], H.PRECISIONS[precision]
            wz, phase = images[base]
            if wz is not None:
                w.w_packed_wz, w.precision_wz = addr(base + ":packed_wz"), wz | (H.WZ_UP_PHASE_IMAGE if phase else 0)
            if skip and not skip_fuse:
                w.precision |= H.SKIP_TWO_CALLS
        return w

    def one(e):
        kind, norm1, conv1, conv2 = {"res": (H.LAYER_RES, ".in_layers.0", ".in_layers.2", ".out_layers.3"),
                                     "attn": (H.LAYER_ATTN, ".norm", ".qkv", ".proj_out"),
                                     "downconv": (H.LAYER_DOWNCONV, None, ".op", None),
                                     "upconv": (H.LAYER_UPCONV, None, ".conv", None)}[e.kind]
        L = H.Layer()
        L.kind, L.updown, L.heads = kind, H.UPDOWN[e.updown], e.heads
        if norm1:
            L.norm1_gamma, L.norm1_beta = addr(e.prefix + norm1 + ".weight"), addr(e.prefix + norm1 + ".bias")
        L.conv1 = weights(e.prefix + conv1)
        if conv2:
            L.conv2 = weights(e.prefix + conv2)
        if e.kind == "res":
            L.film_off = film_off[e.prefix]
            L.norm2_gamma, L.norm2_beta = addr(e.prefix + ".out_layers.0.weight"), addr(e.prefix + ".out_layers.0.bias")
            L.skip = weights(e.prefix + ".skip_connection", skip=True)
        return L

    in_sizes = [len(blk) for blk in topo.input[1:]]
    out_sizes = [len(blk) for blk in topo.output]
    layers = [one(e) for blk in topo.input[1:] for e in blk] + [one(e) for e in topo.middle] \
        + [one(e) for blk in topo.output for e in blk]
    arr = (H.Layer * len(layers))(*layers)
    ins = (C.c_int32 * max(1, len(in_sizes)))(*in_sizes)
    outs = (C.c_int32 * max(1, len(out_sizes)))(*out_sizes)
    d = H.UnetDesc()
    d.n_layers, d.layers = len(layers), arr
    d.n_input_blocks, d.input_block_layers = len(in_sizes), ins
    d.n_middle_layers = len(topo.middle)
    d.n_output_blocks, d.output_block_layers = len(out_sizes), outs
    d.first = weights(topo.input[0][0].prefix)
    d.out_gamma, d.out_beta = addr("out.0.weight"), addr("out.0.bias")
    d.out = weights("out.2")
    d.film, d.planar = int(film), int(planar)
    d.in_channels, d.cin_pad = in_channels, cin_pad
    d.arithmetic = H.PRECISIONS[precision]
    return d, (arr, ins, outs)


class UNetEngine:
    """Executes one model on one device.  `layers` is unet.py's topology."""

    def __init__(self, topo, params, model_channels, film, device, precision="f32", in_channels=2, planar=True,
                 winograd=True, step_graph=False):
        """precision: "f32" = exact fp32 MFMA everywhere; "f16x3" = every conv evaluates
        each fp32 product as three f16 MFMAs (fp32-equivalent accuracy, see
        include/ddpm3d.h); "f16" = one f16 MFMA per product (the reference's --use_fp16);
        "bf16" = one bf16 MFMA per product AND the residual stream stored in bf16."""
        if precision not in H.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(H.PRECISIONS))
        self.precision = precision
        # replay a captured hipGraph of the forward instead of issuing its launches one by one (_Plan._replay)
        self.step_graph = step_graph
        # let the library replay its plan (ddpm3d_unet_forward, one call per forward) instead of issuing the plan's
        # launches from Python; the Python replay stays the one that is instrumented (bench.py)
        self.native_plan = False
        self.native_plans = collections.OrderedDict()
        self._native_desc = None
        self.lib = H.load()
        self.topo = topo
        self.device = device
        self.mc = model_channels
        self.film = film  # use_scale_shift_norm
        self.p = params    # name -> device fp32 tensor
        self.plans = collections.OrderedDict()   # (N, D, H, W) -> _Plan, least recently used first
        self.split_above = {}                    # (D, H, W) -> largest batch one launch can address
        st = H.stream()
        self.conv = {}
        self.winograd = winograd
        # planar: the SuperRes first conv reads x and low_res as two single-channel volumes; otherwise
        # the input is an ordinary (N, in_channels, ...) tensor, padded to 16 channels at the edge
        if planar and in_channels != 2:
            raise ValueError("the planar first conv reads ONE image and ONE low_res channel (got in_channels=%d)"
                             % in_channels)
        self.planar = planar
        self.in_channels = in_channels
        self.cin_pad = (in_channels + 15) // 16 * 16
        first = topo.input[0][0].prefix
        # QKVAttention ("new order", unet.py:361-389) splits the qkv conv's 3C outputs as q | k | v, each
        # heads x ch wide; the attention kernel reads the legacy layout (per head: q | k | v).  Same
        # arithmetic either way, so the conv's output channels are permuted once, here, at pack time.
        qkv_perm = {}
        if getattr(topo, "new_attention_order", False):
            for e in topo.all_layers():
                if e.kind == "attn":
                    Cn, ch = e.cin, e.cin // e.heads
                    leg = torch.arange(3 * Cn)
                    h, part, i = leg // (3 * ch), (leg // ch) % 3, leg % ch
                    qkv_perm[e.prefix + ".qkv"] = (part * Cn + h * ch + i).to(device)
        params = dict(params)
        for base, perm in qkv_perm.items():
            params[base + ".weight"] = params[base + ".weight"][perm].contiguous()
            params[base + ".bias"] = params[base + ".bias"][perm].contiguous()
        self.p = params
        self.up_phase, self.skip_fuse = switches(precision, winograd)
        self.shapes = conv_shapes({k: tuple(v.shape) for k, v in params.items()}, first, None if planar else self.cin_pad)
        images = winograd_images(topo, self.shapes, precision, winograd, self.up_phase)
        for base, (Cout, Cin, k) in self.shapes.items():
            t = params[base + ".weight"]
            if t.dim() == 5:
                w = t
            elif k == 3:
                w = torch.zeros(Cout, t.shape[1], 3, 3, 3, dtype=t.dtype, device=t.device)
                w[:, :, 1] = t
            else:
                w = t.reshape(Cout, t.shape[1], 1, 1, 1)
            if w.shape[1] != Cin:       # (the first conv's zero channels)
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, Cin - w.shape[1]))
            self.conv[base] = PackedConv(w, params[base + ".bias"], H.PRECISIONS[precision], st)
            wz, phase = images[base]
            if wz is not None:
                self.conv[base].wz = PackedConv(w, params[base + ".bias"], wz, st)
                if phase:
                    self.conv[base].wz.pack_up_phase(w, st)
        # fuse every ResBlock's emb_layers Linear into one [total, ted] matrix
        self.film_off, self.film_total = film_offsets(topo, {k: tuple(v.shape) for k, v in params.items()})
        ws, bs = [], []
        for prefix in self.film_off:
            b = params[prefix + ".emb_layers.1.bias"]
            if not film:
                # additive embedding: h = conv1(.) + emb_out, so the Linear's bias also
                # carries conv1's bias and its output row is conv1's per-sample bias
                b = b + params[prefix + ".in_layers.2.bias"]
            ws.append(params[prefix + ".emb_layers.1.weight"].float())
            bs.append(b.float())
        self.ted = 4 * model_channels
        # frequency table of timestep_embedding, evaluated on the host exactly as the
        # reference does (nn.py:113-115: th.exp(...) on CPU, then .to(device))
        half = model_channels // 2
        self.freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32)
                               / half).to(device)
        self.emb_w = torch.cat(ws, 0).contiguous()
        self.emb_b = torch.cat(bs, 0).contiguous()
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------ timestep path
    def film_rows(self, t_float, y=None):
        """[R] timesteps (float, original-process index) [+ [R] int64 class labels] -> [R, film_total]."""
        lib, st, p = self.lib, H.stream(), self.p
        R = t_float.numel()
        dev = self.device
        temb = torch.empty(R, self.mc, dtype=torch.float32, device=dev)
        e1 = torch.empty(R, self.ted, dtype=torch.float32, device=dev)
        e2 = torch.empty(R, self.ted, dtype=torch.float32, device=dev)
        rows = torch.empty(R, self.film_total, dtype=torch.float32, device=dev)
        H.check(lib.ddpm3d_timestep_embedding(H.ptr(t_float), R, self.mc, H.ptr(self.freqs), H.ptr(temb), st))
        H.check(lib.ddpm3d_linear(H.ptr(temb), R, self.mc, H.ptr(p["time_embed.0.weight"]),
                                  H.ptr(p["time_embed.0.bias"]), self.ted, 0, H.ptr(e1), self.ted, st))
        H.check(lib.ddpm3d_linear(H.ptr(e1), R, self.ted, H.ptr(p["time_embed.2.weight"]),
                                  H.ptr(p["time_embed.2.bias"]), self.ted, 1, H.ptr(e2), self.ted, st))
        if y is not None:
            # emb = time_embed(.) + label_emb(y), unet.py:703-705
            table = p["label_emb.weight"]
            H.check(lib.ddpm3d_add_embedding(H.ptr(e2), H.ptr(table), H.ptr(y), R, self.ted, table.shape[0], st))
        H.check(lib.ddpm3d_linear(H.ptr(e2), R, self.ted, H.ptr(self.emb_w), H.ptr(self.emb_b),
                                  self.film_total, 1, H.ptr(rows), self.film_total, st))
        return rows

    # ------------------------------------------------------------ plan building
    MAX_PLANS = 4   # a plan owns every activation buffer of its shape; keep the last few shapes only

    def _cached(self, plans, cls, key):
        pl = plans.get(key)
        if pl is None:
            while len(plans) >= self.MAX_PLANS:
                # drop the least recently used shape (its launches are stream-ordered before anything
                # the caching allocator hands the memory to next)
                plans.popitem(last=False)
            pl = plans[key] = cls(self, *key)
        else:
            plans.move_to_end(key)
        return pl

    def plan(self, N, D, Hh, W):        # replayed from Python
        return self._cached(self.plans, _Plan, (N, D, Hh, W))

    def native(self, N, D, Hh, W):      # replayed by the library
        return self._cached(self.native_plans, _NativePlan, (N, D, Hh, W))

    def _addr(self, name):
        base, _, what = name.partition(":")
        pc = self.conv.get(base)
        return H.ptr({"packed": pc.w, "bias": pc.b, "packed_wz": pc.wz and pc.wz.w}[what] if what else self.p[name])

    def native_desc(self):
        """struct ddpm3d_unet_desc of this model (built once, kept with its ctypes arrays; borrows the engine's tensors)"""
        if self._native_desc is None:
            self._native_desc = unet_desc(self.topo, self.shapes, self.film_off, self._addr, self.precision, self.film,
                                          self.planar, self.in_channels, self.cin_pad, self.winograd, self.up_phase,
                                          self.skip_fuse)
        return self._native_desc[0]

    def forward(self, x, low_res, film_rows, film_stride, out=None):
        """x, low_res: (N,1,D,H,W) device fp32.  film_rows: device tensor whose row n
        (stride film_stride floats; 0 = one row shared by the batch) holds the
        fused emb_layers output for sample n.  Returns (N, Cout, D, H, W)."""
        N, _, D, Hh, W = x.shape
        # The kernels address a tensor with 32-bit byte offsets and the C ABI refuses (before
        # launching anything for that conv) a batch whose tensors pass 4 GiB: such a batch runs as
        # two halves, recursively (>= 32 volumes of 64^3 on the published network).
        if N > self.split_above.get((D, Hh, W), 1 << 30):
            return self._forward_halves(x, low_res, film_rows, film_stride, out)
        try:
            # (a batch that cannot be addressed is refused while its plan is being built, at the first
            # conv whose tensors pass 4 GiB: the planner sizes every conv with the C ABI's own rule, before
            # the arena is allocated)
            if self.native_plan:
                return self.native(N, D, Hh, W).run(x, low_res, film_rows, film_stride, out)
            pl = self.plan(N, D, Hh, W)
            return pl.run(x, low_res, film_rows, film_stride, out)
        except H.Ddpm3dError as e:
            if N == 1 or e.code != H.E_2BIG:
                raise
        self.plans.pop((N, D, Hh, W), None)
        self.split_above[(D, Hh, W)] = min(self.split_above.get((D, Hh, W), 1 << 30), N - 1)
        return self._forward_halves(x, low_res, film_rows, film_stride, out)

    def _forward_halves(self, x, low_res, film_rows, film_stride, out):
        N = x.shape[0]
        res = out
        h = (N + 1) // 2
        for a, b in ((0, h), (h, N)):
            rows = film_rows if film_stride == 0 else film_rows.reshape(-1)[a * film_stride:]
            part = self.forward(x[a:b].contiguous(), None if low_res is None else low_res[a:b].contiguous(),
                                rows, film_stride, None if res is None else res[a:b])
            if res is None:
                res = torch.empty((N,) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
                res[a:b] = part
        return res


def plan_records(lib, handle):
    """the step records of a created C plan (ddpm3d_unet_plan_steps)"""
    n = lib.ddpm3d_unet_plan_steps(handle, None, 0)
    if n < 0:
        raise H.Ddpm3dError(n, lib.ddpm3d_unet_last_error().decode())
    recs = (H.PlanStep * n)()
    lib.ddpm3d_unet_plan_steps(handle, recs, n)
    return recs


def replay_list(lib, recs):
    """Translate a C plan's step records into what the Python replay walks: `steps`, a list of (entry, args) in launch
    order, args a mutable list ending in the stream slot; the arguments that belong to a forward call (`first_desc`,
    `last_desc`, `absmax_args`, `pad_args`, `film_patches`, `bias_patches`, from the records' role flags); and
    `conv_meta`, step index -> (kernel family, algorithmic FLOPs) of the launches that are timed.  Conv steps are views
    of the plan's own descriptors: they are valid as long as the C plan is.  Nothing is decided here."""
    # film_patches: gn_finalize arg lists whose film pointer is per call; bias_patches: (conv desc, film offset) of the
    # additive-embedding conv1 bias rows; absmax_args / pad_args: stand-ins where the plan has no such step
    pl = types.SimpleNamespace(steps=[], conv_meta={}, film_patches=[], bias_patches=[], first_desc=None, last_desc=None,
                               absmax_args=[0, 0], pad_args=[0])
    name = C.create_string_buffer(64)
    for r in recs:
        i, o, n = [v or 0 for v in r.in_], [v or 0 for v in r.out], list(r.n)
        if r.kind == H.STEP_CONV:
            d = H.ConvDesc.from_address(r.conv)
            # measurement bookkeeping: 2 FLOPs per MAC, and the kernel family the library routes the descriptor to
            flops = 2.0 * d.N * d.D * d.H * d.W * d.Cout * d.Cin * d.ksize ** 3
            H.check(lib.ddpm3d_conv_kernel_family(C.byref(d), name, 64))
            if r.skip:
                sk = H.ConvSkip.from_address(r.skip)
                flops += 2.0 * d.N * d.D * d.H * d.W * d.Cout * (sk.C0 + sk.C1)     # conv2's family; both convs' FLOPs
                fn, args = lib.ddpm3d_conv3d_skip, [C.byref(d), C.byref(sk), 0]
            else:
                fn, args = lib.ddpm3d_conv3d, [C.byref(d), 0]
            pl.conv_meta[len(pl.steps)] = (name.value.decode(), flops)
            if r.flags & H.STEP_X:
                pl.first_desc = d
            if r.flags & H.STEP_OUT:
                pl.last_desc = d
            if r.flags & H.STEP_FILM_BIAS:
                pl.bias_patches.append((d, r.film_off))
        elif r.kind == H.STEP_FINALIZE:
            fn, args = lib.ddpm3d_gn_finalize, [i[0], n[0], n[1], i[1], n[2], n[3], n[4], n[5], r.count, r.eps, i[2], i[3],
                                                0, 0, r.film_off, o[0], o[1], o[2], 0]
            if r.flags & H.STEP_FILM:
                pl.film_patches.append(args)
        elif r.kind == H.STEP_ABSMAX:
            fn, args = lib.ddpm3d_absmax, [0, 0, n[0], n[1], o[0], 0]
            pl.absmax_args = args
        elif r.kind == H.STEP_PAD:
            fn, args = lib.ddpm3d_ncdhw_to_ndhwc_pad, [0, n[0], n[1], n[2], n[3], o[0], 0]
            pl.pad_args = args
        elif r.kind == H.STEP_POOL_ACT:
            fn, args = lib.ddpm3d_pool_act, [i[0], i[1], i[2]] + n[:7] + [o[0], n[7], 0]
            pl.conv_meta[len(pl.steps)] = ("pool_act", 0.0)      # timed with the convs (no FLOPs of its own)
        elif r.kind == H.STEP_ATTENTION:
            fn, args = lib.ddpm3d_attention_p, [i[0]] + n[:5] + [i[1], n[5], n[6], o[0], 0]
            # two T x T x ch products per head (the reference's count_flops_attn, unet.py:308-325)
            pl.conv_meta[len(pl.steps)] = ("attention_ch%d" % n[3], 4.0 * n[0] * n[2] * float(n[1]) ** 2 * n[3])
        else:
            raise RuntimeError("unknown plan step kind %d" % r.kind)
        pl.steps.append((fn, args))
    return pl


class _PlanBase:
    """A plan of the library (include/ddpm3d.h: ddpm3d_unet_plan -- libddpm3d is the only planner) in an arena this
    object owns, and what it offers the engine: run() = enqueue one forward (launch by launch, or as one captured
    graph).  The two subclasses are the two replayers of its step list."""
    timing = None

    def __init__(self, eng, N, D, Hh, W):
        self.eng, self.N = eng, N
        self.graphs = {}        # film-row mode -> (captured forward, its static input buffers): _replay()
        lib, desc = eng.lib, eng.native_desc()
        need = lib.ddpm3d_unet_plan_bytes(C.byref(desc), N, D, Hh, W)
        if need == 0:
            msg = lib.ddpm3d_unet_last_error().decode()
            # (the sizing query has no status code: a tensor beyond 32-bit offsets is what makes the engine split a batch)
            raise H.Ddpm3dError(H.E_2BIG if "4 GiB" in msg else H.E_INVAL, msg)
        self.arena, self.act_bytes = torch.empty(need, dtype=torch.uint8, device=eng.device), need   # every buffer of the plan
        self.handle = C.c_void_p()
        rc = lib.ddpm3d_unet_plan_create(C.byref(desc), N, D, Hh, W, H.ptr(self.arena), need, C.byref(self.handle))
        if rc != 0:
            raise H.Ddpm3dError(rc, lib.ddpm3d_unet_last_error().decode())
        self.out_buf = torch.empty((N, eng.conv["out.2"].Cout, D, Hh, W), dtype=torch.float32, device=eng.device)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.eng.lib.ddpm3d_unet_plan_destroy(self.handle)
        except Exception:
            pass

    def run(self, x, low_res, film_rows, film_stride, out=None):
        H.require_device(x, "x")
        if self.eng.planar:
            H.require_device(low_res, "low_res")
        if self.eng.step_graph and self.timing is None:
            return self._replay(x, low_res, film_rows, film_stride, out)
        target = out if out is not None else self.out_buf
        self._enqueue(x.data_ptr(), low_res.data_ptr() if self.eng.planar else 0, film_rows.data_ptr(), film_stride,
                      target.data_ptr())
        return target

    # ---- step graph ----------------------------------------------
    def _replay(self, x, low_res, film_rows, film_stride, out):
        """One hipGraph launch instead of ~230 kernel launches issued from the host (what the reference does as
        ~600 ATen launches per step, gaussian_diffusion.py:522-535).  The C ABI only enqueues, so a forward is
        captured once per (plan, film-row mode) on torch's capture stream; what changes from step to step -- x,
        the conditioning volume, the step's film row -- is copied into buffers the graph was captured on (two or
        three small device-to-device copies in front of the launch), and the result is the plan's own output
        buffer.  Same kernels, same arguments, same order as the eager replay: bit-identical results."""
        eng, N = self.eng, self.N
        shared = film_stride == 0
        g = self.graphs.get(shared)
        if g is None:
            ft = eng.film_total
            st = {"x": torch.empty_like(x),
                  "lr": torch.empty_like(low_res) if eng.planar else None,
                  "film": torch.empty((1 if shared else N) * ft, dtype=torch.float32, device=x.device)}
            args = (st["x"].data_ptr(), st["lr"].data_ptr() if eng.planar else 0, st["film"].data_ptr(),
                    0 if shared else ft, self.out_buf.data_ptr())
            self._stage_inputs(st, x, low_res, film_rows, film_stride)
            self._enqueue(*args)                    # eager once: lazy per-kernel attributes, first-touch of every buffer
            torch.cuda.current_stream().synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._enqueue(*args)
            g = self.graphs[shared] = (graph, st)
        graph, st = g
        self._stage_inputs(st, x, low_res, film_rows, film_stride)
        graph.replay()
        if out is not None:
            out.copy_(self.out_buf)
            return out
        return self.out_buf

    def _stage_inputs(self, st, x, low_res, film_rows, film_stride):
        ft = self.eng.film_total
        st["x"].copy_(x)
        if st["lr"] is not None:
            # (every call: a caller's temporary may come back at the same address with other contents, so there is
            # no safe way to tell "the same conditioning volume" -- the copy is 1 MiB per 64^3 volume, ~3 us)
            st["lr"].copy_(low_res)
        flat = film_rows.reshape(-1)
        if film_stride == 0:
            st["film"].copy_(flat[:ft])
        else:
            st["film"].view(self.N, ft).copy_(torch.as_strided(flat, (self.N, ft), (film_stride, 1)))


class _NativePlan(_PlanBase):
    """The plan replayed by the library itself: ddpm3d_unet_forward issues every launch of the list in one call.
    Same calls in the same order as _Plan below: bit-identical results."""

    def _enqueue(self, xptr, lrptr, fptr, film_stride, outptr):
        rc = self.eng.lib.ddpm3d_unet_forward(self.handle, xptr, lrptr, fptr, film_stride, outptr, H.stream())
        if rc != 0:
            raise H.Ddpm3dError(rc, self.eng.lib.ddpm3d_unet_last_error().decode())


class _Plan(_PlanBase):
    """The plan replayed from Python: the library's step list (replay_list), issued launch by launch -- with HIP
    events around every conv when `timing` is a list (bench.py, tools/).  The descriptors in `steps` are views of memory
    the C plan owns: keep the _Plan itself for as long as they are used (the engine keeps the last MAX_PLANS plans)."""

    def __init__(self, eng, N, D, Hh, W):
        super().__init__(eng, N, D, Hh, W)
        vars(self).update(vars(replay_list(eng.lib, plan_records(eng.lib, self.handle))))
        # bf16 / f16 modes: the residual stream is stored in 16 bits (f16: as the reference's --use_fp16 torso, unet.py:1035)
        self.half_dtype = {"bf16": torch.bfloat16, "f16": torch.float16}.get(eng.precision)
        # only the split-f16 arithmetic scales its operands from in_bound (api.hip: prec_scaled)
        self.scaled = eng.precision in ("f16x3", "f16")

    # ---- execution -----------------------------------------------------------
    def _enqueue(self, xptr, lrptr, fptr, film_stride, outptr):
        """Patch the per-call pointers into the descriptors and enqueue every step on the current stream."""
        st = H.stream()
        if self.eng.planar:
            self.first_desc.src0 = xptr
            self.first_desc.src1 = lrptr
            self.absmax_args[0], self.absmax_args[1] = xptr, lrptr
        else:
            self.absmax_args[0] = self.pad_args[0] = xptr
        for a in self.film_patches:
            a[12], a[13] = fptr, film_stride
        for dsc, off in self.bias_patches:
            dsc.bias = fptr + 4 * off
            dsc.bias_stride_n = film_stride
        self.last_desc.out = outptr
        if self.timing is None:
            for fn, args in self.steps:
                args[-1] = st
                rc = fn(*args)
                if rc != 0:
                    H.check(rc)
        else:
            # measurement replay: HIP events (on the stream the kernels are enqueued on)
            # around every conv launch
            for i, (fn, args) in enumerate(self.steps):
                args[-1] = st
                meta = self.conv_meta.get(i)
                if meta is not None:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                rc = fn(*args)
                if rc != 0:
                    H.check(rc)
                if meta is not None:
                    e1.record()
                    self.timing.append((meta[0], meta[1], e0, e1))
