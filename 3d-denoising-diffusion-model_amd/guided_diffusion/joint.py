"""
Joint patch sampling: one reverse-diffusion state for the whole volume.

The reference samples every 96^3 patch on its own and Hann-blends the finished
patches once (scripts/test.py:100-146).  Where patches overlap, that blend
averages independent posterior draws, which shrinks their spread by
sqrt(sum w_p^2) / sum w_p (down to 1/sqrt(8) where eight patches meet), so a
per-voxel std map carries the imprint of the tiling.  Here the patches are
sampled jointly instead: x_t and every step's noise are whole-volume canvases
(patches.joint_geometry), each step cuts them into the overlapping patches
(ddpm3d_joint_gather), runs the network and the existing fused step kernel on
the patches, and blends the updated patches back with weights that sum to 1 at
every voxel (ddpm3d_joint_blend).  Every patch sees the same x_t and the same
noise in an overlap, and the noise is never averaged.  The forwards per volume
are unchanged (patches x steps); DESIGN.md 3.7.

Both kernels are HIP (csrc/tiling.hip); there is no host fallback.  A sliding
geometry (patches.joint_geometry(..., min_overlap=N): any volume size, any
number of patches per axis) takes the same two steps through
ddpm3d_tiles_gather / ddpm3d_tiles_blend, the same two kernels instantiated
to keep the starts in device memory and to visit only the patches that cover
a voxel.
"""

import collections
import ctypes
import weakref

import numpy as np
import torch as th

from . import _hip as H
from . import dist_util
from . import gaussian_diffusion as gd
from . import guidance
from . import logger
from . import patches


_DEVICE_GEOMETRY = weakref.WeakKeyDictionary()       # JointGeometry -> {device: _Descriptor}

# entries: "ddpm3d_joint" or "ddpm3d_tiles"; args: what their _gather and _blend take for the geometry (the blend
# after them blend_args); keep: the arrays that args point into
_Descriptor = collections.namedtuple("_Descriptor", "entries args blend_args keep")


def _descriptor(geom, device):
    """What the geometry's two entries take on `device`, built once per geometry and device: a ddpm3d_joint_starts
    and, for the blend, the three weight tables back to back for the fixed grid (min_overlap is None); for a sliding
    geometry a ddpm3d_tiling of the host starts, their device copy, the per-coordinate {first covering patch, count}
    lookup (patches.axis_cover) and the tables."""
    cache = _DEVICE_GEOMETRY.setdefault(geom, {})
    key = str(device)
    if key not in cache:
        Dc, Hh, W = geom.canvas
        axes = ((geom.x_starts, Hh), (geom.y_starts, W), (geom.z_starts, Dc))
        host = [np.ascontiguousarray(starts, dtype=np.int32) for starts, _ in axes]
        for starts in host:
            if geom.min_overlap is None and len(starts) > H.JOINT_MAX_STARTS:
                raise ValueError("at most %d patches per axis, got %d" % (H.JOINT_MAX_STARTS, len(starts)))
        tables = th.from_numpy(np.concatenate([np.ascontiguousarray(t, dtype=np.float64).ravel()
                                               for t in (geom.a_x, geom.a_y, geom.a_z)])).to(device)
        if geom.min_overlap is None:
            s = H.JointStarts()
            for n, arr, starts in zip(("nx", "ny", "nz"), (s.xs, s.ys, s.zs), host):
                setattr(s, n, len(starts))
                arr[:len(starts)] = starts.tolist()
            cache[key] = _Descriptor("ddpm3d_joint", s, (H.ptr(tables),), (tables,))
        else:
            cover = np.concatenate([patches.axis_cover(starts, extent, geom.res) for starts, extent in axes])
            dev = [th.from_numpy(a).to(device) for a in (np.concatenate(host), np.ascontiguousarray(cover))]
            t = H.Tiling()
            for a, arr in enumerate(host):
                t.n[a] = len(arr)
                t.starts[a] = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            t.d_starts, t.d_cover, t.d_tables = dev[0].data_ptr(), dev[1].data_ptr(), tables.data_ptr()
            cache[key] = _Descriptor("ddpm3d_tiles", t, (), (host, dev, tables))
    return cache[key]


def _device_tiling(geom, device):
    """The cached ddpm3d_tiling of a sliding geometry on `device` (the GPU tests put their own host starts beside
    its device tables)."""
    return _descriptor(geom, device).args


def gather(canvas, geom, first_patch=0, n_patches=None, out=None):
    """(B, Dc, H, W) float32 canvases on the device -> (n_patches * B, 1, res, res, res) patches first_patch ..
    first_patch + n_patches - 1 of the geometry, patch-major, draw-minor.  A copy: bit-exact."""
    H.require_device(canvas, "canvas")
    if canvas.dim() != 4 or tuple(canvas.shape[1:]) != tuple(geom.canvas):
        raise ValueError("canvas of shape %s, expected (B, %d, %d, %d)"
                         % ((tuple(canvas.shape),) + tuple(geom.canvas)))
    B, r = int(canvas.shape[0]), geom.res
    n = geom.n_patches - first_patch if n_patches is None else int(n_patches)
    if out is None:
        out = th.empty((max(n, 0) * B, 1, r, r, r), dtype=th.float32, device=canvas.device)
    else:
        H.require_device(out, "out")
        if out.numel() != n * B * r ** 3:
            raise ValueError("out holds %d elements, %d patches x %d draws need %d"
                             % (out.numel(), n, B, n * B * r ** 3))
    Dc, Hh, W = geom.canvas
    d = _descriptor(geom, canvas.device)
    with th.cuda.device(canvas.device):
        H.check(getattr(H.load(), d.entries + "_gather")(H.ptr(canvas), B, Dc, Hh, W, r, d.args, int(first_patch), n,
                                                         H.ptr(out), H.stream()))
    return out


def blend(patch_values, geom, num_draws=1, out=None):
    """(P * B, 1, res, res, res) float32 patches (patch-major, draw-minor) -> (B, Dc, H, W) canvases with
    patches.joint_blend's arithmetic, bit for bit."""
    H.require_device(patch_values, "patch_values")
    B, r = int(num_draws), geom.res
    if patch_values.numel() != geom.n_patches * B * r ** 3:
        raise ValueError("patches of shape %s, expected (%d, 1, %d, %d, %d)"
                         % (tuple(patch_values.shape), geom.n_patches * B, r, r, r))
    if out is None:
        out = th.empty((B,) + tuple(geom.canvas), dtype=th.float32, device=patch_values.device)
    else:
        H.require_device(out, "out")
        if tuple(out.shape) != (B,) + tuple(geom.canvas):
            raise ValueError("out of shape %s, expected %s" % (tuple(out.shape), (B,) + tuple(geom.canvas)))
    Dc, Hh, W = geom.canvas
    d = _descriptor(geom, patch_values.device)
    with th.cuda.device(patch_values.device):
        H.check(getattr(H.load(), d.entries + "_blend")(H.ptr(patch_values), B, Dc, Hh, W, r, d.args, *d.blend_args,
                                                        H.ptr(out), H.stream()))
    return out


def _canvas_of(volume, geom, device):
    """A (D, H, W) volume (numpy or tensor, D <= Dc) as one zero-extended (1, Dc, H, W) float32 canvas on `device`.
    A sliding geometry's canvas extends H and W to one patch as well."""
    vol = th.as_tensor(volume, dtype=th.float32)
    Dc, Hh, W = geom.canvas
    if geom.min_overlap is not None:
        fits = vol.dim() == 3 and all(v <= c for v, c in zip(vol.shape, geom.canvas))
    else:
        fits = vol.dim() == 3 and tuple(vol.shape[1:]) == (Hh, W) and vol.shape[0] <= Dc
    if not fits:
        raise ValueError("low_res volume of shape %s does not fit the canvas %s"
                         % (tuple(vol.shape), tuple(geom.canvas)))
    canvas = th.zeros((1, Dc, Hh, W), dtype=th.float32, device=device)
    canvas[0, :vol.shape[0], :vol.shape[1], :vol.shape[2]] = vol.to(device)
    return canvas


def sample_loop_progressive(diffusion, model, low_res_volume, geom, kind="ddpm", num_draws=1, batch_size=1,
                            noise=None, step_noise=None, clip_denoised=True, eta=0.0, device=None, trace=None,
                            noise_key=None, guide=None):
    """Joint DDPM ("ddpm") or DDIM ("ddim", any eta) sampling of one volume; yields, per reverse step,
    {"sample", "pred_xstart"}: (K, Dc, H, W) canvases on the device, K = num_draws.

    low_res_volume  the (D, H, W) conditioning volume (zero-extended to the canvas here)
    geom            patches.joint_geometry(volume.shape, res)
    batch_size      patches per network call; a call's batch is batch_size patches x K draws, patch-major
    noise           the (K, Dc, H, W) start canvas x_T; step_noise: the per-step noise canvases, a sequence in draw
                    order or a callable (k, like) as in the independent loops.  Without them, draw d takes all its
                    noise from dist_util.volume_generator(0, draw=d), one whole canvas at a time, so the result
                    depends on neither the batch size nor the world size.
    noise_key       a gaussian_diffusion.NoiseKey of K streams, one per draw's canvas (draw_key(seed, K) names them
                    dist_util.noise_stream(0, d)): x_T is its draw 0 (unless `noise` is given) and step k reads draw
                    k + 1 inside the step kernel, indexed by the canvas voxel, so every patch that covers a voxel reads
                    the same normal there.  No noise canvas is drawn, held or gathered.  Not with `step_noise`.
    trace           a metrics.StepTrace: every step's blended pred_xstart canvases are its estimates, so its target
                    and weight are (Dc, H, W) or (K, Dc, H, W) canvases (weight 0 outside the volume)
    guide           a guidance.LowPassPull without a measurement of its own: on the steps it is active on, every patch's
                    x_start prediction is pulled towards that patch's own conditioning (the low_res patch the network
                    reads) before the step, and the blend averages the pulled patches.  Within a radius of a patch face
                    the low-pass is one-sided; the Hann weights are small there.
    With several ranks, batch b runs on rank b mod W; the ranks exchange their updated patches once per round and
    every rank blends all of them: all ranks hold the same canvas after every step, bit for bit."""
    if kind not in ("ddpm", "ddim"):
        raise ValueError("joint sampling implements the DDPM and DDIM steps, not %r (DPM-Solver++ keeps its history "
                         "per patch and is not part of the joint loop)" % (kind,))
    K, bs = int(num_draws), max(1, int(batch_size))
    if not 1 <= K <= H.MAX_DRAWS:
        raise ValueError("num_draws must be in 1..%d, got %d" % (H.MAX_DRAWS, K))
    diffusion._check_key(noise_key, step_noise)
    guidance.check_guide(guide)
    if guide is not None and guide.measurement is not None:
        raise ValueError("joint sampling pulls every patch towards its own conditioning: a guide with a measurement of "
                         "its own is refused")
    if noise_key is not None and (noise_key.n != K or noise_key.origin is not None):
        raise ValueError("noise_key must hold one stream per draw (%d) and no geometry of its own" % K)
    if device is None:
        params = getattr(model, "parameters", None)
        device = next(params()).device if params is not None else dist_util.dev()
    device = th.device(device)
    if device.type != "cuda":
        raise RuntimeError("sampling runs on HIP kernels only; got device %s" % device)
    P, r = geom.n_patches, geom.res
    cshape = (K,) + tuple(geom.canvas)
    rounds = dist_util.partition((P + bs - 1) // bs)
    world = dist_util.world_size()

    def rows(b):                                  # batch b's rows of the (P * K) patch buffers
        return b * bs * K, min((b + 1) * bs, P) * K

    with th.no_grad(), th.cuda.device(device):
        if noise_key is None:
            gens = [dist_util.volume_generator(0, seed=10, device=device, draw=d) for d in range(K)]

            def draw():
                return th.stack([th.randn(cshape[1:], device=device, generator=g) for g in gens])

            patch_key = None
        else:
            # row p * K + d of the patch buffers: stream of draw d, origin (z, h, w) of patch p -- one small table
            origin = np.repeat(np.asarray([(zs, xs, ys) for xs, ys, zs in geom.grid], dtype=np.int32), K, axis=0)
            patch_key = gd.NoiseKey(noise_key.seed, noise_key.streams.repeat(P),
                                    origin=th.from_numpy(origin).to(device), patch=(r, r, r), canvas=geom.canvas)

        img = noise if noise is not None else (draw() if noise_key is None else noise_key.fill(0, cshape))
        H.require_device(img, "noise")
        if tuple(img.shape) != cshape:
            raise ValueError("noise of shape %s, expected %s" % (tuple(img.shape), cshape))
        xg = th.empty((bs * K, 1, r, r, r), dtype=th.float32, device=device)
        zg = th.empty_like(xg) if noise_key is None else None
        sliding = geom.min_overlap is not None
        if sliding:
            # any number of patches: the conditioning patches are cut per batch, not held for the whole volume
            low_canvas = _canvas_of(low_res_volume, geom, device)
            lrg, lr1 = th.empty_like(xg), (th.empty((bs, 1, r, r, r), dtype=th.float32, device=device) if K > 1
                                           else None)
            logger.log("joint sampling: %d patches x %d draws, %.2f GB for the updated patches of a step"
                       % (P, K, 2 * P * K * r ** 3 * 4 / 1e9))

            def cond(lo, hi):
                n = (hi - lo) // K
                if K == 1:
                    return gather(low_canvas, geom, lo, n, out=lrg[:n])
                gather(low_canvas, geom, lo // K, n, out=lr1[:n])
                lrg[:hi - lo].view(n, K, -1).copy_(lr1[:n].view(n, 1, -1).expand(n, K, -1))
                return lrg[:hi - lo]
        else:
            low_res = gather(_canvas_of(low_res_volume, geom, device), geom).repeat_interleave(K, dim=0)

            def cond(lo, hi):
                return low_res[lo:hi]
        nets = {}                                 # one step table per batch size (there are at most two)
        for b in rounds:
            if b is not None:
                lo, hi = rows(b)
                if hi - lo not in nets:
                    nets[hi - lo] = diffusion._step_model(model, (hi - lo, 1, r, r, r), {"low_res": cond(lo, hi)},
                                                          device)
        updated = th.empty((2, P * K, 1, r, r, r), dtype=th.float32, device=device)   # sample, pred_xstart
        block = th.zeros((2, bs * K, 1, r, r, r), dtype=th.float32, device=device) if world > 1 else None
    prev = None

    for k, i in enumerate(range(diffusion.num_timesteps - 1, -1, -1)):
        with th.no_grad(), th.cuda.device(device):
            if noise_key is None:
                z = draw() if step_noise is None else diffusion._draw_noise(step_noise, k, img)
                diffusion._check_noise(z, img)
            for b in rounds:
                if b is not None:
                    lo, hi = rows(b)
                    t_all, net = nets[hi - lo]
                    x = xg[:hi - lo]
                    gather(img, geom, lo // K, (hi - lo) // K, out=x)
                    dst = updated[:, lo:hi] if world == 1 else block[:, :hi - lo]
                    lr = cond(lo, hi)
                    mo = net(x, i, lr)
                    xs = diffusion._guided_x0(guide, lr, mo, x, t_all[i], i, clip_denoised)
                    if noise_key is None:
                        zb = zg[:hi - lo]
                        gather(z, geom, lo // K, (hi - lo) // K, out=zb)
                        diffusion._update(kind, mo, x, t_all[i], zb, clip_denoised, eta, out=(dst[0], dst[1]), xstart=xs)
                    else:
                        diffusion._update(kind, mo, x, t_all[i], None, clip_denoised, eta, out=(dst[0], dst[1]),
                                          noise_key=patch_key.rows(lo, hi), draw=k + 1, xstart=xs)
                if world > 1:
                    for bb, blk in dist_util.gather_round(block, b):
                        lo, hi = rows(bb)
                        updated[:, lo:hi].copy_(blk[:, :hi - lo])
            out = {"sample": blend(updated[0], geom, K), "pred_xstart": blend(updated[1], geom, K)}
            if trace is not None:
                prev = diffusion._trace_step(trace, out, prev, i)
        yield out
        img = out["sample"]


def draw_key(seed, num_draws=1, device=None):
    """The NoiseKey of a joint loop of `num_draws` draws: draw d's canvas is stream dist_util.noise_stream(0, d)."""
    return gd.NoiseKey(seed, [dist_util.noise_stream(0, d) for d in range(int(num_draws))], device=device)


def sample_loop(diffusion, model, low_res_volume, geom, **kwargs):
    """The final canvases, (K, Dc, H, W), of sample_loop_progressive."""
    final = None
    for final in sample_loop_progressive(diffusion, model, low_res_volume, geom, **kwargs):
        pass
    return final["sample"]
