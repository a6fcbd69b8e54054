"""
GPU tier of joint patch sampling: the two kernels against their numpy restatements bit for bit, the C
refusals, one joint step against the same step on the whole canvas (the noise is not attenuated in overlaps), the
joint DDPM / DDIM loops against a loop built from the CPU oracle's network, step and patches.joint_blend, the
independence of the result from the batch size, and the inference script's --joint_patches path on one and two ranks.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import PKG, rel_err
from guided_diffusion import _hip as H
from guided_diffusion import joint, patches
from guided_diffusion import script_util as su
from guided_diffusion import synth
from oracle import sampler_ref, schedule_ref, unet_ref
from tiling_ref import np_blend as _np_blend, np_gather as _np_gather

pytestmark = pytest.mark.gpu

PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True,
                 use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)

# the issue's four geometries (every y start a multiple of 4: the 16-byte forms) and two whose y starts ([0, 13, 26]
# in a W of 42, [0, 14, 28] in a W of 44) force the scalar forms
ALIGNED = [(130, 200, 200, 96), (20, 40, 40, 16), (10, 40, 16, 16), (16, 40, 16, 16)]
MISALIGNED = [(20, 40, 42, 16), (20, 40, 44, 16)]


def build(over, resp=""):
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(over)
    fl["timestep_respacing"] = resp
    model, diff = su.sr_create_model_and_diffusion(**fl)
    sd = {k: torch.from_numpy(synth.synth_param(k, tuple(v.shape))) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model.to("cuda").eval()
    return model, diff, sd


@pytest.mark.parametrize("D,Hh,W,res,B", [g + (b,) for g in ALIGNED[1:] + MISALIGNED for b in (1, 3)]
                         + [ALIGNED[0] + (2,)])
def test_kernels_equal_their_numpy_restatements_bit_for_bit(D, Hh, W, res, B):
    geom = patches.joint_geometry((D, Hh, W), res)
    rng = np.random.default_rng(D + W + B)
    canvases = rng.standard_normal((B,) + geom.canvas).astype(np.float32)
    want = _np_gather(canvases, geom)
    dev = torch.from_numpy(canvases).cuda()
    got = joint.gather(dev, geom)
    assert got.shape == (geom.n_patches * B, 1, res, res, res)
    assert np.array_equal(got.cpu().numpy(), want)
    # a range of patches lands where the whole gather puts it
    first, n = geom.n_patches // 3, max(1, geom.n_patches // 2)
    part = joint.gather(dev, geom, first, n)
    assert np.array_equal(part.cpu().numpy(), want[first * B:(first + n) * B])

    rows = rng.standard_normal(want.shape).astype(np.float32)                 # patches that disagree in overlaps
    blended = joint.blend(torch.from_numpy(rows).cuda(), geom, B)
    assert blended.shape == (B,) + geom.canvas
    assert np.array_equal(blended.cpu().numpy(), _np_blend(rows, geom, B))
    # and a pointer that is not 16-byte aligned takes the scalar forms to the same bits
    if res < 96:
        flat = torch.empty(dev.numel() + 1, device="cuda")[1:]
        flat.copy_(dev.reshape(-1))
        assert np.array_equal(joint.gather(flat.reshape(dev.shape), geom).cpu().numpy(), want)
        prow = torch.empty(rows.size + 1, device="cuda")[1:]
        prow.copy_(torch.from_numpy(rows).reshape(-1))
        assert np.array_equal(joint.blend(prow.reshape(rows.shape), geom, B).cpu().numpy(),
                              blended.cpu().numpy())


def _starts(xs, ys, zs, counts=None):
    s = H.JointStarts()
    s.nx, s.ny, s.nz = counts or (len(xs), len(ys), len(zs))
    for arr, vals in ((s.xs, xs), (s.ys, ys), (s.zs, zs)):
        for i, v in enumerate(vals[:H.JOINT_MAX_STARTS]):
            arr[i] = v
    return s


@pytest.mark.parametrize("entry,over,st", [
    (e, o, s) for e in ("gather", "blend") for o, s in [
        (dict(src=None), {}), (dict(out=None), {}), (dict(res=0), {}), (dict(res=1025), {}),
        (dict(B=0), {}), (dict(B=H.MAX_DRAWS + 1), {}),
        ({}, dict(xs=list(range(8)), counts=(9, 3, 2))), ({}, dict(ys=[0, 12, 40])), ({}, dict(zs=[-1, 4])),
        ({}, dict(ys=[0, 12, 25])), ({}, dict(zs=[0, 5])),                   # a patch that leaves the canvas
    ]] + [("blend", dict(tables=None), {}), ("blend", {}, dict(xs=[0, 24])), ("blend", {}, dict(zs=[0])),
          ("blend", dict(W=57), {})])
def test_c_entries_refuse_bad_arguments_and_launch_nothing(entry, over, st):
    """Real device buffers, filled with a sentinel: a refused call returns DDPM3D_EINVAL and leaves the output alone."""
    geom = patches.joint_geometry((20, 40, 40), 16)
    canvases = torch.full((2,) + geom.canvas, 7.0, device="cuda")
    rows = torch.full((geom.n_patches * 2, 1, 16, 16, 16), 7.0, device="cuda")
    tables = torch.zeros(40 + 40 + 20, dtype=torch.float64, device="cuda").repeat(8)
    sa = dict(xs=geom.x_starts, ys=geom.y_starts, zs=geom.z_starts)
    sa.update(st)
    s = _starts(**sa)
    lib = H.load()
    a = dict(src=H.ptr(canvases if entry == "gather" else rows), B=2, Dc=20, H=40, W=40, res=16, starts=s)
    if entry == "gather":
        a.update(first_patch=0, n_patches=geom.n_patches, out=H.ptr(rows), stream=H.stream())
    else:
        a.update(tables=H.ptr(tables), out=H.ptr(canvases), stream=H.stream())
    a.update(over)
    rc = getattr(lib, "ddpm3d_joint_" + entry)(*a.values())
    assert rc == H.E_INVAL and lib.ddpm3d_last_error().decode().startswith("joint_%s:" % entry)
    torch.cuda.synchronize()
    assert bool((canvases == 7.0).all()) and bool((rows == 7.0).all())


def _zeros(x, t, low_res=None):
    return torch.zeros_like(x)


@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.5)])
def test_one_joint_step_equals_the_step_on_the_whole_canvas(kind, eta):
    """Noise is not attenuated: with a network that returns zeros (no learned variance, no clipping) the step is
    elementwise, so every covering patch holds the value the whole-canvas step computes and the blend's weights sum
    to 1 within a few 2^-53: only the final rounding can move a voxel, outermost planes included."""
    _, diff, _ = build(dict(TINY, learn_sigma=False), "10")
    geom = patches.joint_geometry((20, 40, 40), 16)
    x, z = (torch.from_numpy(a).cuda() for a in synth.synth_noise((1,) + geom.canvas, 2, seed=31))
    low = np.zeros((20, 40, 40), dtype=np.float32)
    gen = joint.sample_loop_progressive(diff, _zeros, low, geom, kind=kind, noise=x, step_noise=[z],
                                        clip_denoised=False, eta=eta, batch_size=4, device="cuda")
    got = next(gen)
    gen.close()
    t = torch.tensor([diff.num_timesteps - 1], device="cuda")                # the first step of the loop: index 9
    assert int(t) > 0
    step = diff.p_sample if kind == "ddpm" else (lambda *a, **k: diff.ddim_sample(*a, eta=eta, **k))
    want = step(_zeros, x[None], t, clip_denoised=False, noise=z[None])
    for key in ("sample", "pred_xstart"):
        a, b = got[key].cpu().numpy(), want[key][0].cpu().numpy()
        ulps = np.abs(a - b) / np.spacing(np.abs(b))
        print("%s %s: max distance %.2f ulp, %d of %d voxels differ" % (kind, key, ulps.max(), (a != b).sum(), a.size))
        assert a.shape == b.shape == (1,) + geom.canvas and ulps.max() <= 1.0
    # the noise term is live: the step's output is not its mean
    assert float((got["sample"] - got["pred_xstart"]).abs().max()) > 0.1


def _oracle_joint_loop(sd, cfg, tmap, tb, geom, low_canvas, draws, kind, learn_sigma=True):
    """The joint loop on the CPU: the oracle's network and step on every patch, patches.joint_blend after every step.
    Returns the canvas after every step."""
    lr = torch.from_numpy(patches.joint_gather(low_canvas, geom))
    img = draws[0]
    T = len(tmap)
    steps = []
    with torch.no_grad():
        for k, i in enumerate(range(T - 1, -1, -1)):
            x = torch.from_numpy(patches.joint_gather(img, geom))
            z = torch.from_numpy(patches.joint_gather(draws[1 + k], geom))
            out = unet_ref.unet_forward(sd, cfg, x, torch.full((x.shape[0],), tmap[i], dtype=torch.long), lr)
            mean, log_var, x0 = sampler_ref.mean_variance(tb, out, x, i, learn_sigma)
            mask = 0.0 if i == 0 else 1.0
            if kind == "ddpm":
                new = mean + mask * torch.exp(0.5 * log_var) * z
            else:                                                             # sampler_ref.ddim_sample_loop, eta = 0
                c = sampler_ref._coef
                eps = (c(tb["sqrt_recip_alphas_cumprod"], i) * x - x0) / c(tb["sqrt_recipm1_alphas_cumprod"], i)
                ab_prev = torch.tensor(c(tb["alphas_cumprod_prev"], i))
                new = x0 * torch.sqrt(ab_prev) + torch.sqrt(1 - ab_prev) * eps
            img = patches.joint_blend(new.numpy(), geom)
            steps.append(img)
    return steps


@pytest.fixture(scope="module")
def tiny():
    model, diff, sd = build(TINY, "10")
    geom = patches.joint_geometry((20, 40, 40), 16)
    assert geom.n_patches == 18
    draws = synth.synth_noise((2,) + geom.canvas, 11, seed=10)               # two draws' worth of canvases
    low = synth.synth_low_res((20, 40, 40), seed=1234)
    return model, diff, sd, geom, draws, low


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_joint_loops_vs_cpu_oracle(tiny, kind):
    """Final canvas of the 10-step joint loops against the oracle loop: the 1e-3 bar of the project's 10-step loops
    (test_sampler_loops_vs_reference_golden).  Then two draws at batch size 4: draw d of the pair is the run with
    draw d's noise alone.  Measured on an MI355X, error after steps 1..10: DDPM 3.0e-6 .. 1.1e-5, 3.5e-5 at the end;
    DDIM (eta = 0, no fresh noise) 2.0e-6 5.3e-6 1.1e-5 2.3e-5 4.0e-5 6.4e-5 1.1e-4 1.8e-4 4.7e-4 4.9e-4: the first
    forward's fp32 difference carried and multiplied along a deterministic trajectory."""
    model, diff, sd, geom, draws, low = tiny
    cfg = unet_ref.sr_config(**TINY)
    tmap, tb = schedule_ref.spaced_schedule(1000, "linear", "10")
    refs = [_oracle_joint_loop(sd, cfg, tmap, tb, geom, low, [d[k] for d in draws], kind) for k in (0, 1)]
    dev = [torch.from_numpy(d).cuda() for d in draws]
    per_step = [o["sample"] for o in joint.sample_loop_progressive(
        diff, model, low, geom, kind=kind, noise=dev[0][:1].contiguous(),
        step_noise=[d[:1].contiguous() for d in dev[1:]])]
    # the error after every step, so that a reader sees rounding carried along the trajectory and not a drift
    print("joint %s, rel err vs CPU oracle after steps 1..10: %s"
          % (kind, " ".join("%.2e" % rel_err(s[0].cpu().numpy(), r) for s, r in zip(per_step, refs[0]))))
    one, refs = per_step[-1], [r[-1] for r in refs]
    err = rel_err(one[0].cpu().numpy(), refs[0])
    print("joint %s, 18 patches of 16^3, 10 steps: rel err vs CPU oracle %.3e" % (kind, err))
    assert one.shape == (1,) + geom.canvas and err < 1e-3
    two = joint.sample_loop(diff, model, low, geom, kind=kind, num_draws=2, batch_size=4, noise=dev[0],
                            step_noise=dev[1:])
    assert two.shape == (2,) + geom.canvas
    for k in (0, 1):
        err = rel_err(two[k].cpu().numpy(), refs[k])
        print("  draw %d of 2 at batch size 4: %.3e" % (k, err))
        assert err < 1e-3
    assert not np.array_equal(two[0].cpu().numpy(), two[1].cpu().numpy())


def test_result_does_not_depend_on_the_batch_size_and_repeats(tiny):
    model, diff, _, geom, draws, low = tiny
    dev = [torch.from_numpy(d[:1]).cuda() for d in draws]

    def run(bs):
        return joint.sample_loop(diff, model, low, geom, batch_size=bs, noise=dev[0],
                                 step_noise=dev[1:]).cpu().numpy()

    a1, a18, b18, b1 = run(1), run(18), run(18), run(1)
    print("batch size 1 vs 18: rel %.3e" % rel_err(a18, a1))
    assert rel_err(a18, a1) < 1e-3                 # conv routes may differ by batch: the loops' parity bar, not bits
    assert np.array_equal(a18, b18) and np.array_equal(a1, b1)
    # the loop's own noise is drawn per canvas, not per batch: the same holds without injected noise
    c1 = joint.sample_loop(diff, model, low, geom, batch_size=1).cpu().numpy()
    c5 = joint.sample_loop(diff, model, low, geom, batch_size=5).cpu().numpy()
    assert rel_err(c5, c1) < 1e-3 and not np.array_equal(c1, a1)


def test_a_step_does_not_synchronise_with_the_host(tiny):
    """No .item() / .cpu() / synchronize() inside a reverse step of a one-rank run: under torch's sync debug mode a
    step after the first (whose set-up may upload tables) raises on any blocking call."""
    model, diff, _, geom, draws, low = tiny
    dev = [torch.from_numpy(d[:1]).cuda() for d in draws]
    gen = joint.sample_loop_progressive(diff, model, low, geom, batch_size=4, noise=dev[0], step_noise=dev[1:])
    next(gen)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = next(gen)
        out = next(gen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        gen.close()
    assert bool(torch.isfinite(out["sample"]).all())


FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3 --joint_patches True").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_joint_patches_npz_end_to_end(tmp_path):
    vol = np.random.default_rng(3).random((20, 40, 40), dtype=np.float32)    # (D, H, W): 3 x 3 x 2 patches of 16^3
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    mod = _script()
    base = ["--base_samples", str(src), "--batch_size", "4"]
    path = mod.main(FLAGS + base + ["--save_dir", str(tmp_path / "one")])
    assert path == str(tmp_path / "one" / "denoised_pet.npz")
    with np.load(path) as z:
        assert z.files == ["arr_0"]
        one = z["arr_0"]
    assert one.shape == (40, 40, 20) and one.dtype == np.float32 and np.isfinite(one).all()      # (H, W, Z)
    # the outermost planes hold real values (the one-shot stitcher writes 0 there)
    for plane in (one[0], one[-1], one[:, 0], one[:, -1], one[:, :, 0], one[:, :, -1]):
        assert np.abs(plane).min() > 0
    with np.load(mod.main(FLAGS + base + ["--save_dir", str(tmp_path / "k3"), "--num_draws", "3"])) as z:
        assert sorted(z.files) == ["arr_0", "std"]
        mean, std = z["arr_0"], z["std"]
    assert mean.shape == std.shape == (40, 40, 20) and std.dtype == np.float32
    assert np.isfinite(mean).all() and np.isfinite(std).all() and std.min() >= 0 and std.max() > 0
    assert np.abs(mean[0]).min() > 0 and np.abs(mean[:, :, -1]).min() > 0 and std[0].max() > 0
    # the mean of three draws is not the single draw
    assert not np.array_equal(mean, one)
    # DDIM takes the same path
    flags = [f if f != "3" else "ddim3" for f in FLAGS]
    with np.load(mod.main(flags + base + ["--save_dir", str(tmp_path / "ddim"), "--use_ddim", "True"])) as z:
        ddim = z["arr_0"]
    assert ddim.shape == (40, 40, 20) and np.isfinite(ddim).all() and not np.array_equal(ddim, one)


def test_script_joint_patches_depth_below_one_patch(tmp_path):
    """A volume thinner than a patch: the canvas is zero-extended along depth and the output cropped back."""
    vol = np.random.default_rng(4).random((10, 40, 16), dtype=np.float32)
    src = tmp_path / "thin.npy"
    np.save(src, vol)
    arr = np.load(_script().main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o")]))["arr_0"]
    assert arr.shape == (40, 16, 10) and np.isfinite(arr).all() and np.abs(arr).min() > 0


def test_update_checks_the_tensors_it_is_told_to_write_into():
    _, diff, _ = build(dict(TINY, learn_sigma=False), "10")
    x, z, mo = (torch.randn(2, 1, 4, 8, 8, device="cuda") for _ in range(3))
    t = torch.tensor([3, 3], device="cuda")
    good = torch.empty_like(x), torch.empty_like(x)
    want = diff._update("ddpm", mo, x, t, z, True)
    got = diff._update("ddpm", mo, x, t, z, True, out=good)
    assert got["sample"] is good[0] and torch.equal(got["sample"], want["sample"])
    assert torch.equal(got["pred_xstart"], want["pred_xstart"])
    strided = torch.empty(2, 1, 4, 8, 16, device="cuda")[..., ::2]
    for bad in ((strided, good[1]), (good[0], strided), (good[0].cpu(), good[1]),
                (good[0].double(), good[1])):
        with pytest.raises(RuntimeError):
            diff._update("ddpm", mo, x, t, z, True, out=bad)
    with pytest.raises(AssertionError):
        diff._update("ddpm", mo, x, t, z, True, out=(good[0][:1], good[1]))


def test_script_joint_patches_tif_in_tif_out(tmp_path):
    """.tif in: denoised_<name>.npz (H, W, Z) plus denoised_<name>.tif and, with draws, denoised_<name>_std.tif, both
    (Z, H, W) float32 like the independent path writes them."""
    from guided_diffusion import tiff_io
    vol = (np.random.default_rng(6).random((20, 24, 24)) * 4000).astype(np.uint16)
    src = tmp_path / "pet.tif"
    tiff_io.imwrite(str(src), vol)
    path = _script().main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o"), "--num_draws", "2"])
    with np.load(path) as z:
        mean, std = z["arr_0"], z["std"]
    tif = tiff_io.imread(str(tmp_path / "o" / "denoised_pet.tif"))
    tif_std = tiff_io.imread(str(tmp_path / "o" / "denoised_pet_std.tif"))
    assert mean.shape == (24, 24, 20) and tif.shape == tif_std.shape == (20, 24, 24) and tif.dtype == np.float32
    assert np.array_equal(tif, mean.transpose(2, 0, 1)) and np.array_equal(tif_std, std.transpose(2, 0, 1))
    assert np.isfinite(tif).all() and std.max() > 0


def test_script_joint_patches_two_ranks_equal_one_rank(tmp_path):
    """Two ranks (a fresh torch.distributed.run child, gloo, both on cuda:0) share each step's forwards and exchange
    the updated patches once per round; the canvas equals the one-rank run at the same batch size bit for bit."""
    import socket
    import subprocess
    import sys

    vol = np.random.default_rng(9).random((20, 40, 40), dtype=np.float32)    # 18 patches, 5 batches of 4: uneven
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    script = os.path.join(PKG, "scripts", "test.py")
    common = FLAGS + ["--base_samples", str(src), "--batch_size", "4", "--num_draws", "2"]
    with np.load(_script().main(common + ["--save_dir", str(tmp_path / "one")])) as z:
        a, sa = z["arr_0"], z["std"]

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), script] + common + [
           "--save_dir", str(tmp_path / "two"), "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(tmp_path / "two" / "denoised_pet.npz") as z:
        b, sb = z["arr_0"], z["std"]
    assert a.shape == b.shape == (40, 40, 20) and np.abs(a).max() > 0 and sa.max() > 0
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
