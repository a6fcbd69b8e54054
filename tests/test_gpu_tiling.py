"""
GPU tier of the gap-free sliding tiling: ddpm3d_tiles_gather / ddpm3d_tiles_blend against their numpy
restatements (patches.joint_gather / joint_blend) and against the fixed-grid entries bit for bit, the C refusals on
real device buffers, and the inference script's --patch_overlap on all three paths: the one-shot blend and --num_draws
against the default run on a volume both grids tile alike, the one-shot blend of a volume the fixed grid cannot tile
against a restatement from per-patch p_sample_loop calls and patches.stitch_patches (one and two ranks, two batch
sizes), the joint loop on more than eight patches per axis, and the warning of the default grid on a volume with gaps.

Every test runs under a time limit of its own (a watchdog ends the process: nothing more is started on a device that
hangs), every child process under its own.
"""

import ctypes
import faulthandler
import importlib.util
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from guided_diffusion import _hip as H
from guided_diffusion import dist_util, joint, patches
from guided_diffusion import script_util as su
from guided_diffusion import synth
from tiling_ref import np_blend as _np_blend, np_gather as _np_gather

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 600


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


TINY = dict(large_size=16, small_size=16, num_channels=32, num_res_blocks=1, num_head_channels=64,
            attention_resolutions="1000", learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True)

# (D, H, W), res, overlap: ten starts along H with W starts [0, 6, 12, 18, 24] (scalar forms); y starts multiples of 4
# (16-byte forms) on a volume the fixed grid cannot tile; two axes shorter than a patch; a W that is no multiple of 4;
# the fixed grid's own geometry; one zero-padded patch
GEOMETRIES = [((20, 70, 40), 16, 10), ((40, 70, 52), 16, 4), ((10, 70, 12), 16, 4), ((30, 100, 33), 16, 7),
              ((24, 40, 40), 16, 4), ((5, 7, 9), 16, 2)]


def _as_sliding(g):
    """The same starts and tables, routed through the tiles entries."""
    return patches.JointGeometry(g.canvas, g.res, g.x_starts, g.y_starts, g.z_starts, g.a_x, g.a_y, g.a_z,
                                 min_overlap=2)


@pytest.mark.parametrize("shape,res,ov,B", [g + (b,) for g in GEOMETRIES for b in (1, 3)]
                         + [((130, 200, 200), 96, 44, 2)])
def test_kernels_equal_their_numpy_restatements_bit_for_bit(shape, res, ov, B):
    geom = patches.joint_geometry(shape, res, min_overlap=ov)
    if shape == (20, 70, 40):
        assert len(geom.x_starts) == 10 and any(y % 4 for y in geom.y_starts)
    rng = np.random.default_rng(sum(shape) + B)
    canvases = rng.standard_normal((B,) + geom.canvas).astype(np.float32)
    want = _np_gather(canvases, geom)
    dev = torch.from_numpy(canvases).cuda()
    got = joint.gather(dev, geom)
    assert got.shape == (geom.n_patches * B, 1, res, res, res)
    assert np.array_equal(got.cpu().numpy(), want)
    first, n = geom.n_patches // 3, max(1, geom.n_patches // 2)
    part = joint.gather(dev, geom, first, n)
    assert np.array_equal(part.cpu().numpy(), want[first * B:(first + n) * B])

    rows = rng.standard_normal(want.shape).astype(np.float32)                 # patches that disagree in overlaps
    blended = joint.blend(torch.from_numpy(rows).cuda(), geom, B)
    assert blended.shape == (B,) + geom.canvas
    assert np.array_equal(blended.cpu().numpy(), _np_blend(rows, geom, B))
    # a pointer that is not 16-byte aligned takes the scalar forms to the same bits
    if res < 96:
        flat = torch.empty(dev.numel() + 1, device="cuda")[1:]
        flat.copy_(dev.reshape(-1))
        assert np.array_equal(joint.gather(flat.reshape(dev.shape), geom).cpu().numpy(), want)
        prow = torch.empty(rows.size + 1, device="cuda")[1:]
        prow.copy_(torch.from_numpy(rows).reshape(-1))
        assert np.array_equal(joint.blend(prow.reshape(rows.shape), geom, B).cpu().numpy(),
                              blended.cpu().numpy())


@pytest.mark.parametrize("D,Hh,W,res,B", [(130, 200, 200, 96, 2), (20, 40, 40, 16, 3), (10, 40, 40, 16, 1),
                                          (16, 24, 40, 16, 2), (20, 40, 42, 16, 3), (20, 40, 44, 16, 1)])
def test_new_entries_equal_the_fixed_grid_entries_bit_for_bit(D, Hh, W, res, B):
    """Fixed-grid geometries whose starts ascend (the tiles entries refuse repeated starts, which the fixed grid
    produces for an axis of exactly one patch: [0, 0, 0]), 16-byte and scalar forms."""
    old = patches.joint_geometry((D, Hh, W), res)
    new = _as_sliding(old)
    rng = np.random.default_rng(D + W)
    canvases = torch.from_numpy(rng.standard_normal((B,) + old.canvas).astype(np.float32)).cuda()
    a, b = joint.gather(canvases, old), joint.gather(canvases, new)
    assert a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(joint.gather(canvases, old, 2, 5), joint.gather(canvases, new, 2, 5))
    rows = torch.from_numpy(rng.standard_normal(tuple(a.shape)).astype(np.float32)).cuda()
    ca, cb = joint.blend(rows, old, B), joint.blend(rows, new, B)
    assert ca.shape == cb.shape == (B,) + old.canvas
    assert np.array_equal(ca.cpu().numpy().view(np.uint32), cb.cpu().numpy().view(np.uint32))


def _descriptor(geom, xs=None, ys=None, zs=None, counts=None, **over):
    """ddpm3d_tiling on real device tables of `geom`, with host starts that may be overridden."""
    dev_t = joint._device_tiling(geom, torch.device("cuda", torch.cuda.current_device()))
    t = H.Tiling()
    keep = []
    for a, vals in enumerate((geom.x_starts if xs is None else xs, geom.y_starts if ys is None else ys,
                              geom.z_starts if zs is None else zs)):
        arr = (ctypes.c_int32 * max(len(vals), 1))(*vals)
        keep.append(arr)
        t.n[a] = len(vals) if counts is None else counts[a]
        t.starts[a] = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))
    t.d_starts, t.d_cover, t.d_tables = dev_t.d_starts, dev_t.d_cover, dev_t.d_tables
    for k, v in over.items():
        setattr(t, k, v)
    return t, keep


@pytest.mark.parametrize("entry,over,st", [
    (e, o, s) for e in ("gather", "blend") for o, s in [
        (dict(src=None), {}), (dict(out=None), {}), (dict(tiling=None), {}), (dict(res=0), {}), (dict(res=1025), {}),
        (dict(B=0), {}), (dict(B=H.MAX_DRAWS + 1), {}),
        (dict(Dc=65536), {}), (dict(H=65534, W=32769), {}),                  # an axis, a plane too large
        ({}, dict(ys=[0, 12, 40])), ({}, dict(zs=[-1, 4])), ({}, dict(ys=[0, 12, 25])), ({}, dict(zs=[0, 5])),
        ({}, dict(xs=[])), ({}, dict(ys=[12, 0, 24])), ({}, dict(d_starts=None)),
    ]] + [("gather", dict(first_patch=-1), {}), ("gather", dict(n_patches=0), {}),
          ("gather", dict(first_patch=17, n_patches=2), {}), ("gather", dict(n_patches=19), {}),
          ("blend", {}, dict(d_tables=None)), ("blend", {}, dict(d_cover=None)),
          ("blend", {}, dict(xs=[0, 24])), ("blend", {}, dict(zs=[0])), ("blend", dict(W=57), {})])
def test_c_entries_refuse_bad_arguments_and_launch_nothing(entry, over, st):
    """Real device buffers, filled with a sentinel: a refused call returns DDPM3D_EINVAL and leaves the output alone."""
    geom = patches.joint_geometry((20, 40, 40), 16, min_overlap=4)
    assert geom.n_patches == 18
    canvases = torch.full((2,) + geom.canvas, 7.0, device="cuda")
    rows = torch.full((geom.n_patches * 2, 1, 16, 16, 16), 7.0, device="cuda")
    t, keep = _descriptor(geom, **st)
    lib = H.load()
    a = dict(src=H.ptr(canvases if entry == "gather" else rows), B=2, Dc=20, H=40, W=40, res=16,
             tiling=ctypes.byref(t))
    if entry == "gather":
        a.update(first_patch=0, n_patches=geom.n_patches, out=H.ptr(rows), stream=H.stream())
    else:
        a.update(out=H.ptr(canvases), stream=H.stream())
    a.update(over)
    rc = getattr(lib, "ddpm3d_tiles_" + entry)(*a.values())
    assert rc == H.E_INVAL and lib.ddpm3d_last_error().decode().startswith("tiles_%s:" % entry)
    torch.cuda.synchronize()
    assert bool((canvases == 7.0).all()) and bool((rows == 7.0).all())


def test_entries_refuse_more_rows_than_they_can_index():
    """nx * ny * nz * B above 2^31 - 1 rows is refused before a launch (the rows of an accepted call are split into
    launches of at most 65535, the grid's z extent)."""
    geom = patches.joint_geometry((20, 40, 40), 16, min_overlap=4)
    starts = list(range(1291))
    t, keep = _descriptor(geom, xs=starts, ys=starts, zs=starts)
    out = torch.full((64,), 7.0, device="cuda")
    lib = H.load()
    rc = lib.ddpm3d_tiles_blend(H.ptr(out), 1, 1306, 1306, 1306, 16, ctypes.byref(t), H.ptr(out), H.stream())
    assert rc == H.E_INVAL and "too many rows" in lib.ddpm3d_last_error().decode()
    rc = lib.ddpm3d_tiles_gather(H.ptr(out), 1, 1306, 1306, 1306, 16, ctypes.byref(t), 0, 1, H.ptr(out), H.stream())
    assert rc == H.E_INVAL and "too many rows" in lib.ddpm3d_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_a_gather_of_more_rows_than_one_launch_holds():
    """1749 x 21 patches of 4^3 for two canvases, 73 458 rows: two launches (65535 + 7923) write what the numpy
    statement writes."""
    shape, res, ov = (4, 1752, 24), 4, 3
    geom = patches.joint_geometry(shape, res, min_overlap=ov)
    B = 2
    assert geom.n_patches * B > 65535
    rng = np.random.default_rng(1)
    canvases = rng.standard_normal((B,) + geom.canvas).astype(np.float32)
    got = joint.gather(torch.from_numpy(canvases).cuda(), geom)
    assert np.array_equal(got.cpu().numpy(), _np_gather(canvases, geom))


# ------------------------------------------------------------------------------------------- the inference script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build(resp):
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(TINY)
    fl["timestep_respacing"] = resp
    model, diff = su.sr_create_model_and_diffusion(**fl)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape)))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    return model, diff


def _restated(vol, grid, res, resp="3"):
    """What the script's one-shot path computes, restated: every patch of `grid` cut with zero padding, sampled on its
    own by p_sample_loop with all of its noise from volume_generator(i), permuted to (H, W, Z) and blended by
    patches.stitch_patches."""
    model, diff = _build(resp)
    dev = torch.device("cuda", torch.cuda.current_device())
    done = []
    for i, (xs, ys, zs) in enumerate(grid):
        cut = vol[zs:zs + res, xs:xs + res, ys:ys + res]
        cond = np.zeros((1, 1, res, res, res), dtype=np.float32)
        cond[0, 0, :cut.shape[0], :cut.shape[1], :cut.shape[2]] = cut
        gen = dist_util.volume_generator(i, seed=10, device=dev)

        def draw(_k=None, _img=None):
            return torch.randn(1, 1, res, res, res, device=dev, generator=gen)

        noise = draw()
        sample = diff.p_sample_loop(model, (1, 1, res, res, res), noise, clip_denoised=True,
                                    model_kwargs={"low_res": torch.from_numpy(cond).to(dev)}, step_noise=draw)
        done.append(sample.permute(0, 1, 3, 4, 2)[0, 0].cpu().numpy())
    return patches.stitch_patches(done, grid, vol.shape, res)


def _off_faces(arr):
    return arr[1:-1, 1:-1, 1:-1]


def test_script_patch_overlap_equals_the_default_run_where_the_grids_agree(tmp_path):
    """24 x 40 x 40 at 16^3: overlap 4 is the fixed grid.  Same grid, same noise keys, same stitch arithmetic (on the
    device instead of the host): the same arr_0, bit for bit; with two draws the same arr_0 and std."""
    vol = np.random.default_rng(3).random((24, 40, 40), dtype=np.float32)
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    mod = _script()
    base = FLAGS + ["--base_samples", str(src), "--batch_size", "4"]
    a = np.load(mod.main(base + ["--save_dir", str(tmp_path / "a")]))["arr_0"]
    with np.load(mod.main(base + ["--save_dir", str(tmp_path / "b"), "--patch_overlap", "4"])) as z:
        assert z.files == ["arr_0"]
        b = z["arr_0"]
    assert a.shape == b.shape == (40, 40, 24) and b.dtype == np.float32 and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    with np.load(mod.main(base + ["--save_dir", str(tmp_path / "c"), "--num_draws", "2"])) as z:
        m0, s0 = z["arr_0"], z["std"]
    with np.load(mod.main(base + ["--save_dir", str(tmp_path / "d"), "--num_draws", "2", "--patch_overlap", "4"])) as z:
        assert sorted(z.files) == ["arr_0", "std"]
        m1, s1 = z["arr_0"], z["std"]
    assert s0.max() > 0 and not np.array_equal(m0, a)
    assert np.array_equal(m0.view(np.uint32), m1.view(np.uint32))
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32))


def test_script_tiles_a_volume_the_fixed_grid_cannot(tmp_path):
    """40 x 70 x 52 at 16^3, overlap 4 (3 x 6 x 4 = 72 patches along D, H, W), batch size 1: arr_0 is the restatement
    bit for bit, no voxel off the six faces is 0; batch size 3 and two ranks give the same bits."""
    shape, res, ov = (40, 70, 52), 16, 4
    vol = np.random.default_rng(11).random(shape, dtype=np.float32)
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    grid = patches.sliding_grid(shape, res, ov)
    assert len(grid) == 72 and any(patches.grid_gaps(shape, res).values())
    want, weight = _restated(vol, grid, res)
    mod = _script()
    common = FLAGS + ["--base_samples", str(src), "--patch_overlap", str(ov)]
    one = np.load(mod.main(common + ["--save_dir", str(tmp_path / "bs1"), "--batch_size", "1"]))["arr_0"]
    assert one.shape == (70, 52, 40) and one.dtype == np.float32 and np.isfinite(one).all()
    assert np.array_equal(one.view(np.uint32), want.view(np.uint32))
    assert np.abs(_off_faces(one)).min() > 0 and _off_faces(weight).min() > 0
    three = np.load(mod.main(common + ["--save_dir", str(tmp_path / "bs3"), "--batch_size", "3"]))["arr_0"]
    print("batch size 3 vs 1: %d of %d voxels differ, max abs %.3g"
          % ((three != one).sum(), one.size, np.abs(three - one).max()))
    assert np.array_equal(three.view(np.uint32), one.view(np.uint32))

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(PKG, "scripts", "test.py")] + common + [
           "--save_dir", str(tmp_path / "two"), "--batch_size", "1", "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    two = np.load(tmp_path / "two" / "denoised_pet.npz")["arr_0"]
    assert np.array_equal(two.view(np.uint32), one.view(np.uint32))


def test_script_dpm_solver_runs_on_the_sliding_grid_and_joint_refuses_it(tmp_path):
    vol = np.random.default_rng(5).random((10, 44, 16), dtype=np.float32)
    src = tmp_path / "pet.npy"
    np.save(src, vol)
    mod = _script()
    flags = [f if f != "3" else "logsnr3" for f in FLAGS]
    arr = np.load(mod.main(flags + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o"), "--patch_overlap",
                                    "4", "--use_dpm_solver", "True"]))["arr_0"]
    assert arr.shape == (44, 16, 10) and np.isfinite(arr).all() and np.abs(_off_faces(arr)).min() > 0
    with pytest.raises(SystemExit):
        mod.main(flags + ["--base_samples", str(src), "--save_dir", str(tmp_path / "p"), "--patch_overlap", "4",
                          "--use_dpm_solver", "True", "--joint_patches", "True"])


def test_default_grid_warns_about_gaps_and_writes_what_it_wrote_before(tmp_path):
    """16 x 60 x 16 at 16^3: the fixed grid's H starts [0, 22, 44] leave rows 16..21 and 38..43 to no patch.  The run
    logs one warning that names --patch_overlap and writes patches.stitch_patches on patch_grid, gaps (zeros)
    included; a volume the grid covers logs no warning."""
    shape, res = (16, 60, 16), 16
    vol = np.random.default_rng(13).random(shape, dtype=np.float32)
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    grid = patches.patch_grid(shape, res)
    want, weight = _restated(vol, grid, res)
    mod = _script()
    got = np.load(mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o")]))["arr_0"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got[16:22] == 0) and np.all(got[38:44] == 0) and np.abs(got[1:15, 1:-1, 1:-1]).min() > 0
    log = open(tmp_path / "o" / "log.txt").read()
    warnings = [ln for ln in log.splitlines() if "WARNING" in ln]
    assert len(warnings) == 1 and "--patch_overlap" in warnings[0] and "12 of 60 along H" in warnings[0]
    np.savez(tmp_path / "ok.npz", vol[:, :40])
    mod.main(FLAGS + ["--base_samples", str(tmp_path / "ok.npz"), "--save_dir", str(tmp_path / "q")])
    assert "WARNING" not in open(tmp_path / "q" / "log.txt").read()


# ------------------------------------------------------------------------------------------- the joint path
def _zeros(x, t, low_res=None):
    return torch.zeros_like(x)


@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.5)])
def test_one_joint_step_on_ten_patches_along_an_axis_equals_the_step_on_the_whole_canvas(kind, eta):
    """test_gpu_joint's statement at 10 x 3 x 2 patches: with a network that returns zeros the step is elementwise, so
    every covering patch holds the whole-canvas step's value and the blend's weights sum to 1 within a few 2^-53: only
    the final rounding can move a voxel."""
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(dict(TINY, learn_sigma=False))
    fl["timestep_respacing"] = "10"
    _, diff = su.sr_create_model_and_diffusion(**fl)
    geom = patches.joint_geometry((20, 70, 24), 16, min_overlap=10)
    assert (len(geom.x_starts), len(geom.y_starts), len(geom.z_starts)) == (10, 3, 2)
    x, z = (torch.from_numpy(a).cuda() for a in synth.synth_noise((1,) + geom.canvas, 2, seed=31))
    low = np.zeros((20, 70, 24), dtype=np.float32)
    gen = joint.sample_loop_progressive(diff, _zeros, low, geom, kind=kind, noise=x, step_noise=[z],
                                        clip_denoised=False, eta=eta, batch_size=7, device="cuda")
    got = next(gen)
    gen.close()
    t = torch.tensor([diff.num_timesteps - 1], device="cuda")
    step = diff.p_sample if kind == "ddpm" else (lambda *a, **k: diff.ddim_sample(*a, eta=eta, **k))
    want = step(_zeros, x[None], t, clip_denoised=False, noise=z[None])
    for key in ("sample", "pred_xstart"):
        a, b = got[key].cpu().numpy(), want[key][0].cpu().numpy()
        ulps = np.abs(a - b) / np.spacing(np.abs(b))
        print("%s %s: max distance %.2f ulp, %d of %d voxels differ" % (kind, key, ulps.max(), (a != b).sum(), a.size))
        assert a.shape == b.shape == (1,) + geom.canvas and ulps.max() <= 1.0
    assert float((got["sample"] - got["pred_xstart"]).abs().max()) > 0.1


def test_joint_run_on_a_volume_the_fixed_grid_cannot_tile_repeats_and_ignores_the_batch_size():
    """4-step DDPM on 40 x 70 x 52 (72 patches of 16^3): the same bits twice, and at batch sizes 1 and 5."""
    model, diff = _build("4")
    shape = (40, 70, 52)
    geom = patches.joint_geometry(shape, 16, min_overlap=4)
    low = synth.synth_low_res(shape, seed=1234)

    def run(bs):
        return joint.sample_loop(diff, model, low, geom, batch_size=bs).cpu().numpy()

    a1, b1, a5 = run(1), run(1), run(5)
    assert a1.shape == (1,) + geom.canvas and np.isfinite(a1).all() and np.abs(a1).min() > 0
    assert np.array_equal(a1.view(np.uint32), b1.view(np.uint32))
    print("batch size 5 vs 1: %d of %d voxels differ, max abs %.3g" % ((a5 != a1).sum(), a1.size, np.abs(a5 - a1).max()))
    assert np.array_equal(a5.view(np.uint32), a1.view(np.uint32))


def test_script_joint_patches_on_the_sliding_grid(tmp_path):
    """--joint_patches True --patch_overlap 4 on a volume with two axes below one patch and one the fixed grid cannot
    tile: the output has the volume's shape and real values on the outermost planes.  Three draws, as in
    test_gpu_joint: clipped voxels are +-1, and an even number of them can cancel to a mean of exactly 0."""
    vol = np.random.default_rng(4).random((10, 70, 12), dtype=np.float32)
    src = tmp_path / "thin.npy"
    np.save(src, vol)
    mod = _script()
    with pytest.raises(ValueError):
        mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "x"), "--joint_patches", "True"])
    with np.load(mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o"), "--joint_patches",
                                   "True", "--patch_overlap", "4", "--num_draws", "3", "--batch_size", "4"])) as z:
        mean, std = z["arr_0"], z["std"]
    assert mean.shape == std.shape == (70, 12, 10) and np.isfinite(mean).all() and np.abs(mean).min() > 0
    assert std.max() > 0
    assert "GB for the updated patches" in open(tmp_path / "o" / "log.txt").read()
