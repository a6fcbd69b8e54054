"""
GPU tier of the per-voxel uncertainty maps: ddpm3d_draw_stitch equals patches.stitch_patches bit
for bit per draw and is bit-repeatable; ddpm3d_draw_moments meets numpy's fp64 mean / std(ddof=1) where the naive
formula cancels; offsets past 2^31 elements land where numpy puts them; `scripts/test.py --num_draws K` equals an
independent reference built in the test from the documented per-(patch, draw) generators, leaves K = 1 unchanged,
and gives the same maps on two ranks as on one.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import PKG
from guided_diffusion import _hip, dist_util, patches, uncertainty

pytestmark = pytest.mark.gpu

FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
DEV = "cuda:0"


def _bar(got, ref):
    """max |got - ref| <= 2e-6 * max |ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.abs(got - ref).max() <= 2e-6 * max(np.abs(ref).max(), 1e-30), np.abs(got - ref).max()


def _hwz(sample_cdhw):
    """one draw as the sampler returns it, (1, Z, H, W) -> the (H, W, Z) patch stitch_patches takes"""
    return np.asarray(sample_cdhw)[0].transpose(1, 2, 0)


def _stitch_on_device(samples, grid, shape_dhw, res, K):
    st = uncertainty.DrawStitcher(shape_dhw, res, K, DEV)
    for i, origin in enumerate(grid):
        st.add(i, torch.from_numpy(samples[i]).to(DEV), origin)
    mean, std, w = st.finish()
    torch.cuda.synchronize()
    return st.acc.cpu().numpy(), w.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy()


@pytest.mark.parametrize("shape_dhw", [(20, 40, 37), (12, 40, 37)])   # the second crops every patch along Z
def test_stitch_is_stitch_patches_bit_for_bit(shape_dhw):
    res, K = 16, 3
    grid = patches.patch_grid(shape_dhw, res)
    rng = np.random.default_rng(11)
    samples = [rng.standard_normal((K, 1, res, res, res)).astype(np.float32) for _ in grid]
    acc, w, mean, std = _stitch_on_device(samples, grid, shape_dhw, res, K)
    D, H, W = shape_dhw
    assert acc.shape == (K, H, W, D) and w.shape == (H, W, D)
    vols = []
    for d in range(K):
        ref, ref_w = patches.stitch_patches([_hwz(s[d]) for s in samples], grid, shape_dhw, res)
        got = np.divide(acc[d], w, out=acc[d].copy(), where=w > 0)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), d
        assert np.array_equal(w.view(np.uint32), ref_w.view(np.uint32))
        vols.append(ref)
    v = np.stack(vols).astype(np.float64)
    _bar(mean, v.mean(0))
    _bar(std, v.std(0, ddof=1))
    assert np.all(mean[w == 0] == 0) and np.all(std[w == 0] == 0) and (w == 0).any()
    again = _stitch_on_device(samples, grid, shape_dhw, res, K)
    for a, b in zip((acc, w, mean, std), again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_stitcher_refuses_patches_out_of_order():
    st = uncertainty.DrawStitcher((16, 16, 16), 16, 2, DEV)
    x = torch.zeros(2, 1, 16, 16, 16, device=DEV)
    st.add(3, x, (0, 0, 0))
    for i in (3, 2):
        with pytest.raises(ValueError):
            st.add(i, x, (0, 0, 0))


def _moments(acc, w):
    """(mean, std) of the device kernel on numpy inputs; w None = the plain stack"""
    a = torch.from_numpy(np.ascontiguousarray(acc)).to(DEV)
    K, n = a.shape[0], a[0].numel()
    mean = torch.empty(n, device=DEV)
    std = torch.empty(n, device=DEV)
    wt = None if w is None else torch.from_numpy(np.ascontiguousarray(w)).to(DEV)
    _hip.check(_hip.load().ddpm3d_draw_moments(_hip.ptr(a), _hip.ptr(wt), K, n, _hip.ptr(mean), _hip.ptr(std),
                                               _hip.stream()))
    return mean.cpu().numpy(), std.cpu().numpy()


def _moments_ref(acc, w):
    if w is None:
        v = acc.astype(np.float64)
    else:
        v = np.stack([np.divide(a, w, out=np.zeros_like(a), where=w > 0) for a in acc]).astype(np.float64)
    return v.mean(0), v.std(0, ddof=1)


@pytest.mark.parametrize("n", [4096 * 3, 1001])          # the float4 form and the one-voxel-per-thread form
@pytest.mark.parametrize("K", [2, 5, 16])
@pytest.mark.parametrize("case", ["random", "large_mean", "weighted_large_mean"])
def test_moments_against_numpy_fp64(n, K, case):
    rng = np.random.default_rng(K * 7 + n)
    w = (rng.random(n) * 3).astype(np.float32)
    w[::7] = 0.0                                          # zero-weight voxels give 0
    if case == "random":
        acc = rng.standard_normal((K, n)).astype(np.float32) * w
    else:                                                 # 1e4 + 1e-3 noise: sum x^2 - (sum x)^2 / K cancels here
        acc = (1e4 + 1e-3 * rng.standard_normal((K, n))).astype(np.float32)
        if case == "weighted_large_mean":
            acc = (acc * w).astype(np.float32)
    for wt in (w, None):
        if case == "weighted_large_mean" and wt is None:
            continue
        mean, std = _moments(acc, wt)
        rm, rs = _moments_ref(acc, wt)
        _bar(mean, rm)
        _bar(std, rs)
        assert np.isfinite(mean).all() and np.isfinite(std).all() and (std >= 0).all()
        if wt is not None:
            assert np.all(mean[w == 0] == 0) and np.all(std[w == 0] == 0)


@pytest.mark.parametrize("weighted", [True, False])
def test_moments_of_constant_draws_are_exactly_zero(weighted):
    rng = np.random.default_rng(2)
    n, K = 4096 + 3, 9
    row = (rng.standard_normal(n) * 1e4).astype(np.float32)
    acc = np.repeat(row[None], K, axis=0)
    w = (rng.random(n) + 0.5).astype(np.float32) if weighted else None
    mean, std = _moments(acc, w)
    assert np.all(std == 0.0) and not np.signbit(std).any()
    ref = np.divide(row, w) if weighted else row
    assert np.array_equal(mean, ref.astype(np.float32))


def test_stitch_offsets_past_two_to_the_31():
    """One origin at the far corner of a volume whose K * H * W * D passes 2^31 elements (about 12 GB on the
    device): the touched voxels of the last draw hold what numpy computes for them, and the moments too."""
    res, K = 16, 3
    D, H, W = 600, 1100, 1100
    assert K * H * W * D > 2 ** 31
    xs, ys, zs = H - res, W - 9, D - 5                    # cropped along W and Z
    rng = np.random.default_rng(4)
    x = rng.standard_normal((K, 1, res, res, res)).astype(np.float32)
    st = uncertainty.DrawStitcher((D, H, W), res, K, DEV)
    st.add(0, torch.from_numpy(x).to(DEV), (xs, ys, zs))
    mean, std, wt = st.finish()
    torch.cuda.synchronize()
    win = patches.hann_window_3d(res)[:, :9, :5]
    w_ref = np.zeros((res, 9, 5), np.float32)
    w_ref += win
    got_w = wt[xs:, ys:, zs:].cpu().numpy()
    assert np.array_equal(got_w.view(np.uint32), w_ref.view(np.uint32))
    vols = []
    for d in range(K):
        a_ref = np.zeros((res, 9, 5), np.float32)
        a_ref += _hwz(x[d])[:, :9, :5] * win
        got = st.acc[d, xs:, ys:, zs:].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), a_ref.view(np.uint32)), d
        vols.append(np.divide(a_ref, w_ref, out=a_ref.copy(), where=w_ref > 0))
    assert float(st.acc[K - 1, :xs].abs().max()) == 0.0 and float(st.acc[K - 1, xs:, :ys].abs().max()) == 0.0
    v = np.stack(vols).astype(np.float64)
    _bar(mean[xs:, ys:, zs:].cpu().numpy(), v.mean(0))
    _bar(std[xs:, ys:, zs:].cpu().numpy(), v.std(0, ddof=1))
    del st, mean, std, wt
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the inference script
def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference(mod, vol, K, bs):
    """The maps built independently of the script's draw path: the documented generator per (patch, draw), the
    sampler on the same N = bs * K patch-major batches, each draw stitched by patches.stitch_patches, numpy mean
    and std(ddof = 1)."""
    from guided_diffusion import synth
    from guided_diffusion.script_util import args_to_dict, sr_create_model_and_diffusion, \
        sr_model_and_diffusion_defaults
    args = mod.create_argparser().parse_args(FLAGS)
    model, diffusion = sr_create_model_and_diffusion(**args_to_dict(args, sr_model_and_diffusion_defaults().keys()))
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape)))
                           for k, v in model.state_dict().items()})
    model.to(DEV).eval()
    res = args.large_size
    low_res, grid = patches.split_volume(vol, res)
    out = {}
    for b in range((len(grid) + bs - 1) // bs):
        idx = list(range(b * bs, min((b + 1) * bs, len(grid))))
        cond = torch.cat([torch.from_numpy(low_res[i:i + 1]).to(DEV) for i in idx for _ in range(K)])
        gens = [dist_util.volume_generator(i, seed=10, device=DEV, draw=d) for i in idx for d in range(K)]
        shape = tuple(cond.shape)

        def draw(_k=None, _img=None):
            return torch.cat([torch.randn(1, *shape[1:], device=DEV, generator=g) for g in gens])

        s = diffusion.p_sample_loop(model, shape, draw(), clip_denoised=True, model_kwargs={"low_res": cond},
                                    step_noise=draw).cpu().numpy()
        for j, i in enumerate(idx):
            out[i] = s[j * K:(j + 1) * K]
    vols, weight = [], None
    for d in range(K):
        v, weight = patches.stitch_patches([_hwz(out[i][d]) for i in range(len(grid))], grid, vol.shape, res)
        vols.append(v)
    v = np.stack(vols).astype(np.float64)
    return v.mean(0), v.std(0, ddof=1), weight


@pytest.mark.parametrize("bs", [1, 2])
def test_script_draws_match_an_independent_reference(tmp_path, bs):
    K = 3
    vol = np.random.default_rng(8).random((20, 40, 24), dtype=np.float32)     # 3 x 3 x 2 patches of 16^3
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    mod = _script()
    path = mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o"), "--batch_size", str(bs),
                             "--num_draws", str(K)])
    with np.load(path) as z:
        assert set(z.files) == {"arr_0", "std"}
        mean, std = z["arr_0"], z["std"]
    assert mean.shape == std.shape == (40, 24, 20) and mean.dtype == std.dtype == np.float32
    rm, rs, w = _reference(mod, vol, K, bs)
    _bar(mean, rm)
    _bar(std, rs)
    assert np.all(std[w == 0] == 0) and np.all(mean[w == 0] == 0) and (w == 0).any()
    # inside, std is 0 exactly where the K draws agree bit for bit (voxels every draw clips to the same bound) and
    # positive everywhere else
    inside = w > 0
    assert np.array_equal(std[inside] > 0, rs[inside] > 0)
    assert (std[inside] > 0).mean() > 0.5


def test_script_tif_writes_the_std_tif_and_one_draw_is_unchanged(tmp_path):
    from guided_diffusion import tiff_io
    vol = (np.random.default_rng(6).random((20, 24, 24)) * 4000).astype(np.uint16)
    src = tmp_path / "pet.tif"
    tiff_io.imwrite(str(src), vol)
    mod = _script()
    path = mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "k2"), "--num_draws", "2"])
    with np.load(path) as z:
        mean, std = z["arr_0"], z["std"]
    tif = tiff_io.imread(str(tmp_path / "k2" / "denoised_pet.tif"))
    tif_std = tiff_io.imread(str(tmp_path / "k2" / "denoised_pet_std.tif"))
    assert np.array_equal(tif, mean.transpose(2, 0, 1)) and np.array_equal(tif_std, std.transpose(2, 0, 1))
    assert np.abs(std).max() > 0

    # --num_draws 1 is the single-draw run: the same file bytes for arr_0, no std key, no std tif
    plain = mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "plain")])
    one = mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "one"), "--num_draws", "1"])
    with np.load(plain) as a, np.load(one) as b:
        assert a.files == b.files == ["arr_0"]
        assert a["arr_0"].tobytes() == b["arr_0"].tobytes()
    assert not os.path.exists(tmp_path / "one" / "denoised_pet_std.tif")


def test_two_rank_draws_equal_one_rank(tmp_path):
    """--num_draws 2 under a two-rank gloo torch.distributed.run child (both ranks on cuda:0): an odd number of
    patches, the maps equal the single-process run's bit for bit."""
    import socket
    import subprocess
    import sys

    vol = np.random.default_rng(9).random((16, 40, 16), dtype=np.float32)     # 3 patches of 16^3 along H
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    script = os.path.join(PKG, "scripts", "test.py")
    common = FLAGS + ["--base_samples", str(src), "--num_draws", "2"]
    with np.load(_script().main(common + ["--save_dir", str(tmp_path / "one")])) as z:
        a_mean, a_std = z["arr_0"], z["std"]

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
        b_mean, b_std = z["arr_0"], z["std"]
    assert a_mean.shape == b_mean.shape == (40, 16, 16)
    assert np.array_equal(a_mean, b_mean) and np.array_equal(a_std, b_std)
    assert np.abs(a_std).max() > 0
