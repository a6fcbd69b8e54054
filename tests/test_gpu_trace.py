"""
GPU tier of the per-step convergence trace: ddpm3d_trace_moments against the numpy fp64 yardstick of
tests/trace_ref.py on both load paths, with every stride and NULL combination, weights with exact zeros and NaN / inf
under them, bit-repeatability and batching; the trace= keyword of the four sampling loops and the joint loop against
the yardstick applied to what their _progressive generators yield, with bit-identical samples; and the inference
script's --trace on its four paths.
"""

import importlib.util
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R
import trace_ref as TR
from conftest import PKG
from guided_diffusion import _hip, joint, metrics, patches
from guided_diffusion import script_util as su
from guided_diffusion import synth
from guided_diffusion.respace import space_timesteps

pytestmark = pytest.mark.gpu

VOXELS = [1, 5, 1024, 1025, 4096, 4099, 2049 * 1024 + 3]      # the last: 1025 parts of two passes each, and a tail


def dev(a, offset=0):
    """a device copy of `a`; with offset = 1 a contiguous view one float past a 16-byte boundary (the scalar path)"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    return view


def gpu_moments(est, prev, target, weight):
    """one ddpm3d_trace_moments call on device tensors est (B, voxels), prev or None, target / weight (voxels,) or
    (B, voxels) or None -> (B, REC) fp64 numpy"""
    lib = _hip.load()
    B, voxels = est.shape
    stride = lambda t: 0 if t is None or t.dim() == 1 else voxels
    need = lib.ddpm3d_trace_moments_workspace_bytes(B, voxels)
    assert need > 0
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    out = torch.full((B, _hip.TR_REC), float("nan"), dtype=torch.float64, device="cuda")
    _hip.check(lib.ddpm3d_trace_moments(_hip.ptr(est), _hip.ptr(prev), _hip.ptr(target), _hip.ptr(weight), B, voxels,
                                        stride(target), stride(weight), _hip.ptr(ws), need, _hip.ptr(out),
                                        _hip.stream()))
    return out.cpu().numpy()


def check_records(got, rec, mag, prev, target, weight, what):
    lim = TR.bound(rec, mag)
    err = np.abs(got - rec)
    worst = float(np.max(err / np.maximum(lim, 1e-300)))
    print("%s: worst |got - ref| / bound %.3g" % (what, worst))
    assert np.isfinite(got).all(), what
    assert np.all(err <= lim), (what, err, lim)
    assert np.array_equal(got[:, TR.N], rec[:, TR.N]), what
    if weight is None:
        assert np.array_equal(got[:, TR.W], rec[:, TR.W]), what
    if target is None:
        assert not got[:, list(TR.NEEDS_TARGET)].any(), what
    if prev is None:
        assert not got[:, TR.SUM_SQ_D].any(), what


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("voxels", VOXELS)
def test_trace_moments_match_numpy_fp64(voxels, B):
    """every stride combination with all inputs, every NULL combination, the scalar path on pointers one float off,
    NaN / inf under the zero weights, N exact, W exact without weights, two calls and a batch row's single call
    give the same bits"""
    full = None
    for own_t, own_w in itertools.product((True, False), repeat=2):
        est, prev, target, weight = TR.make_case(B, voxels, seed=voxels % 1000 + 10 * B + 2 * own_t + own_w,
                                                 own_target=own_t, own_weight=own_w)
        if voxels >= 1024:
            assert 0 < (weight == 0).mean() < 1 and (np.abs(est) >= 1).any()
        rec, mag = TR.moments(est, prev, target, weight)
        pe, pp, pt = TR.poison(est, prev, target, weight)
        assert voxels < 1024 or np.isnan(pe).any()
        got = gpu_moments(dev(pe), dev(pp), dev(pt), dev(weight))
        check_records(got, rec, mag, prev, target, weight, "target %s, weight %s" % (("own" if own_t else "shared"),
                                                                                    ("own" if own_w else "shared")))
        if own_t and own_w:
            full = (est, prev, target, weight, pe, pp, pt, rec, mag, got)
    est, prev, target, weight, pe, pp, pt, rec, mag, got = full
    # the same bits on a second call, and on pointers one float past a 16-byte boundary against the yardstick
    assert np.array_equal(gpu_moments(dev(pe), dev(pp), dev(pt), dev(weight)), got)
    off = gpu_moments(dev(pe, 1), dev(pp, 1), dev(pt, 1), dev(weight, 1))
    check_records(off, rec, mag, prev, target, weight, "one float off")
    assert np.array_equal(off, gpu_moments(dev(pe, 1), dev(pp, 1), dev(pt, 1), dev(weight, 1)))
    # row b of a batch is the call on estimate b alone
    for b in range(B):
        single = gpu_moments(dev(pe[b:b + 1]), dev(pp[b:b + 1]), dev(pt[b]), dev(weight[b]))
        assert np.array_equal(single[0], got[b]), b
    # every NULL combination (the poisoned inputs only where a weight hides them)
    for use_p, use_t, use_w in itertools.product((True, False), repeat=3):
        if use_p and use_t and use_w:
            continue
        args = (pe if use_w else est, (pp if use_w else prev) if use_p else None,
                (pt if use_w else target) if use_t else None, weight if use_w else None)
        clean = (est, prev if use_p else None, target if use_t else None, weight if use_w else None)
        r, m = TR.moments(*clean)
        check_records(gpu_moments(*(dev(a) for a in args)), r, m, clean[1], clean[2], clean[3],
                      "prev %d target %d weight %d" % (use_p, use_t, use_w))


def test_trace_moments_with_nothing_counted_and_through_python():
    x = torch.full((2, 1, 4, 4, 4), float("nan"), device="cuda")
    tr = metrics.StepTrace(target=torch.zeros(1, 4, 4, 4, device="cuda"), weight=torch.zeros_like(x))
    tr.add(x, None, 7, 2)
    tr.add(x, x, 3, 2)
    rec = tr.records()
    assert rec.shape == (2, 2, _hip.TR_REC) and not rec.any() and tr.t == [7, 3]
    assert all(v is None for k, v in tr.figures(1.0)[1].items() if k != "weight")
    with pytest.raises(ValueError, match="does not fit"):
        tr.add(x, x, 0, 2)
    with pytest.raises(ValueError, match="shape"):
        metrics.StepTrace(target=torch.zeros(4, 4, device="cuda")).add(x, None, 0, 1)


# ------------------------------------------------------------------------------------------------ the loops
TINY = dict(large_size=16, small_size=16, num_channels=32, num_res_blocks=1, num_head_channels=64,
            attention_resolutions="1000", learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True,
            timestep_respacing="3")
SHAPE = (2, 1, 16, 16, 16)


@pytest.fixture(scope="module")
def tiny():
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(TINY)
    model, diff = su.sr_create_model_and_diffusion(**fl)
    model.load_state_dict({k: torch.from_numpy(synth.synth_param(k, tuple(v.shape)))
                           for k, v in model.state_dict().items()})
    model.to("cuda").eval()
    draws = [torch.from_numpy(a).cuda() for a in synth.synth_noise(SHAPE, 4, seed=10)]
    low = torch.from_numpy(synth.synth_low_res(SHAPE, seed=1234)).cuda()
    return model, diff, draws, low


def _own(shape, seed):
    """own targets in [-1, 1] and random weights with exact zeros, of the loop's x shape"""
    rng = np.random.default_rng(seed)
    target = rng.uniform(-1, 1, shape).astype(np.float32)
    weight = rng.uniform(0.01, 1, shape).astype(np.float32)
    weight[rng.random(shape) < 0.3] = 0.0
    return target, weight


def _check_trace(tr, preds, target, weight, t_want, what):
    rec = tr.records()
    B = preds[0].shape[0]
    assert rec.shape == (len(preds), B, _hip.TR_REC) and tr.t == t_want, (rec.shape, tr.t, t_want)
    flat = lambda a: a.reshape(B, -1)
    for k, x in enumerate(preds):
        r, m = TR.moments(flat(x), flat(preds[k - 1]) if k else None, flat(target), flat(weight))
        check_records(rec[k], r, m, k or None, target, weight, "%s step %d" % (what, k))
        assert rec[k][:, TR.N].min() > 0 and (k == 0 or rec[k][:, TR.SUM_SQ_D].min() > 0)


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm_solver", "ddim_reverse"])
def test_loop_trace_is_the_yardstick_on_what_the_generator_yields(tiny, kind):
    """every trace row equals the yardstick applied to the pred_xstart the _progressive generator yields (the
    previous one as prev), t is the original timestep of each row, and the samples are bit-identical with and without
    trace="""
    model, diff, draws, low = tiny
    kw = dict(model_kwargs={"low_res": low})
    T = diff.num_timesteps
    t_desc = sorted(space_timesteps(1000, "3"), reverse=True)
    assert T == 3 and list(diff.timestep_map) == t_desc[::-1]
    if kind == "ddim_reverse":
        name, args, t_want = "ddim_reverse_sample_loop", (model, draws[0]), t_desc[::-1]
    else:
        name = {"ddpm": "p_sample_loop", "ddim": "ddim_sample_loop", "dpm_solver": "dpm_solver_sample_loop"}[kind]
        args, t_want = (model, SHAPE), t_desc
        kw.update(noise=draws[0])
        if kind == "dpm_solver":
            kw.update(order=2)
        else:
            kw.update(step_noise=draws[1:])
    steps = list(getattr(diff, name + "_progressive")(*args, **kw))
    preds = [s["pred_xstart"].cpu().numpy() for s in steps]
    target, weight = _own(SHAPE, seed=5)
    tr = metrics.StepTrace(target=dev(target), weight=dev(weight))
    traced = getattr(diff, name)(*args, trace=tr, **kw)
    assert torch.equal(traced, steps[-1]["sample"]) and torch.equal(traced, getattr(diff, name)(*args, **kw))
    _check_trace(tr, preds, target, weight, t_want, kind)
    # the _progressive form takes it too; one shared target and no weight
    shared = metrics.StepTrace(target=dev(target[0]))
    again = [s["sample"] for s in getattr(diff, name + "_progressive")(*args, trace=shared, **kw)]
    assert torch.equal(again[-1], traced)
    full = np.ones(SHAPE, dtype=np.float32)
    _check_trace(shared, preds, np.broadcast_to(target[0], SHAPE), full, t_want, kind + ", shared target")
    figs = shared.figures(data_range=2.0)
    assert figs[0]["delta_rms"] is None and all(f["psnr"] is not None and f["weight"] == 2 * 16 ** 3 for f in figs)


def test_joint_loop_trace(tiny):
    """one volume, K = 2 draws: the traced estimate is the blended pred_xstart canvas, the weight a canvas that is 0
    outside the volume"""
    model, diff, _, _ = tiny
    vol = synth.synth_low_res((20, 16, 12), seed=77)
    geom = patches.joint_geometry(vol.shape, 16, min_overlap=6)
    assert geom.canvas == (20, 16, 16) and geom.n_patches == 2
    cshape = (2,) + tuple(geom.canvas)
    target, weight = _own(cshape, seed=6)
    weight[:, :, :, 12:] = 0.0
    kw = dict(kind="ddpm", num_draws=2, batch_size=1)
    steps = list(joint.sample_loop_progressive(diff, model, vol, geom, **kw))
    preds = [s["pred_xstart"].cpu().numpy() for s in steps]
    tr = metrics.StepTrace(target=dev(target), weight=dev(weight))
    traced = joint.sample_loop(diff, model, vol, geom, trace=tr, **kw)
    assert torch.equal(traced, steps[-1]["sample"])
    _check_trace(tr, preds, target, weight, sorted(space_timesteps(1000, "3"), reverse=True), "joint")


# ------------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
ROW_KEYS = {"step", "t", "psnr", "nrmse", "mae", "bias", "mean", "std", "delta_rms", "clipped"}
ERR_KEYS = ("psnr", "nrmse", "mae", "bias")


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    d = tmp_path_factory.mktemp("trace_scans")
    target = R.phantom((24, 40, 40), seed=4)
    np.savez(d / "pet.npz", R.noisy(target, 0.1, seed=4))
    np.savez(d / "full.npz", target)
    base = FLAGS + ["--base_samples", str(d / "pet.npz")]
    return base, base + ["--target_samples", str(d / "full.npz"), "--metrics_mask_threshold", "0.1"]


def _run(flags, save):
    path = _script().main(flags + ["--save_dir", str(save)])
    read = lambda name: open(os.path.join(str(save), name), "rb").read()
    trace = json.loads(read("trace_pet.json")) if os.path.exists(os.path.join(str(save), "trace_pet.json")) else None
    return path, read, trace


def _mse(row, L):
    return L * L / 10.0 ** (row["psnr"] / 10.0)


def _check_file(trace, sampler, pooling, with_target=True):
    assert trace["sampler"] == sampler and trace["pooling"] == pooling and trace["steps"] == 3
    assert [r["step"] for r in trace["rows"]] == [0, 1, 2]
    assert [r["t"] for r in trace["rows"]] == sorted(space_timesteps(1000, "3"), reverse=True)
    for k, r in enumerate(trace["rows"]):
        assert set(r) == ROW_KEYS
        assert (r["delta_rms"] is None) == (k == 0)
        for key in ("mean", "std", "clipped") + (ERR_KEYS if with_target else ()):
            assert r[key] is not None and np.isfinite(r[key]), (k, key)


def test_script_trace_leaves_the_other_files_alone_and_ignores_the_batch_size(scans, tmp_path):
    _, scored = scans
    plain, read_plain, none = _run(scored, tmp_path / "plain")
    assert none is None
    path, read, trace = _run(scored + ["--trace", "True"], tmp_path / "traced")
    assert open(plain, "rb").read() == open(path, "rb").read()               # the .npz: byte for byte as without
    assert read_plain("metrics_pet.json") == read("metrics_pet.json")
    _check_file(trace, "ddpm", "patch")
    rep = json.loads(read("metrics_pet.json"))
    assert trace["n_voxels"] == rep["denoised"]["n_voxels"] > 0
    assert trace["data_range"] == rep["denoised"]["data_range"] and trace["mask_threshold"] == 0.1
    assert trace["target"] == rep["target"]
    log = read("log.txt").decode()
    assert len(re.findall(r"^ *step +\d+ +t +\d+ ", log, re.M)) == 3 and "saved trace to" in log and "saved trace to" not in read_plain("log.txt").decode()
    _, read4, _ = _run(scored + ["--trace", "True", "--batch_size", "4"], tmp_path / "bs4")
    assert read4("trace_pet.json") == read("trace_pet.json")                 # pooled per (patch, draw): byte for byte


def test_script_trace_on_the_sliding_grid_with_draws(scans, tmp_path):
    _, scored = scans
    _, read, trace = _run(scored + ["--trace", "True", "--patch_overlap", "6", "--num_draws", "2", "--batch_size", "3",
                                    "--use_dpm_solver", "True"], tmp_path / "o")
    _check_file(trace, "dpm_solver", "patch")
    rep = json.loads(read("metrics_pet.json"))
    assert trace["n_voxels"] == rep["denoised"]["n_voxels"] > 0 and trace["draws"] == 2


def test_script_joint_ddim_trace_ends_on_the_metrics_row(scans, tmp_path):
    """at t = 0 with eta = 0 the step kernel's sample is x0 * 1 + 0 * eps: the written volume is the last pred_xstart
    canvas bit for bit, and only the summation order separates the last trace row from the metrics file's row.
    Bound: n 2^-52 relative (for the bias relative to the MAE), n the counted voxels; mse is taken from psnr and the
    data range on both sides."""
    _, scored = scans
    _, read, trace = _run(scored + ["--trace", "True", "--joint_patches", "True", "--use_ddim", "True"],
                          tmp_path / "o")
    _check_file(trace, "ddim", "canvas")
    den = json.loads(read("metrics_pet.json"))["denoised"]
    last, n, L = trace["rows"][-1], den["n_voxels"], den["data_range"]
    assert trace["n_voxels"] == n
    tol = n * 2.0 ** -52
    figures = {"mse": (_mse(last, L), _mse(den, L), _mse(den, L)), "mae": (last["mae"], den["mae"], den["mae"]),
               "nrmse": (last["nrmse"], den["nrmse"], den["nrmse"]), "bias": (last["bias"], den["bias"], den["mae"])}
    for key, (a, b, scale) in figures.items():
        print("%s: trace %.17g metrics %.17g, relative %.3g (bound %.3g)" % (key, a, b, abs(a - b) / scale, tol))
    for key, (a, b, scale) in figures.items():
        assert abs(a - b) <= tol * scale, key


def test_script_patch_trace_is_never_below_the_blended_error(scans, tmp_path):
    """Jensen: the share-weighted error of the patches before blending is at least the blended volume's"""
    _, scored = scans
    _, read, trace = _run(scored + ["--trace", "True", "--use_ddim", "True"], tmp_path / "o")
    _check_file(trace, "ddim", "patch")
    den = json.loads(read("metrics_pet.json"))["denoised"]
    a, b = _mse(trace["rows"][-1], den["data_range"]), _mse(den, den["data_range"])
    print("mse of the patches %.9g, of the blended volume %.9g, ratio %.9g" % (a, b, a / b))
    assert a >= b


def test_script_trace_without_a_target(scans, tmp_path):
    base, _ = scans
    _, read, trace = _run(base + ["--trace", "True"], tmp_path / "o")
    _check_file(trace, "ddpm", "patch", with_target=False)
    assert trace["target"] is None and trace["data_range"] is None
    assert all(r[k] is None for r in trace["rows"] for k in ERR_KEYS)
    cover = patches.blend_cover(patches.patch_grid((24, 40, 40), 16), (24, 40, 40), 16)
    assert trace["n_voxels"] == int(cover.sum())


def test_script_trace_two_ranks_equal_one(scans, tmp_path):
    """one two-rank run (gloo, both ranks on one device) on the sliding path: its trace file is the one-rank file,
    byte for byte"""
    import socket
    import subprocess
    import sys
    _, scored = scans
    flags = scored + ["--trace", "True", "--patch_overlap", "6", "--batch_size", "3"]
    _, read, _ = _run(flags, tmp_path / "one")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(PKG, "scripts", "test.py")] + flags + [
           "--save_dir", str(tmp_path / "two"), "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(tmp_path / "two" / "trace_pet.json", "rb").read() == read("trace_pet.json")
    assert open(tmp_path / "two" / "denoised_pet.npz", "rb").read() == read("denoised_pet.npz")
