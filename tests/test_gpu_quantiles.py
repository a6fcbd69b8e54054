"""
Posterior quantile maps and rank calibration on the GPU (csrc/quantiles.hip): ddpm3d_draw_quantiles
against numpy's fp64 quantiles within the bound of its three fp32 roundings, its sorting network proven for K <= 16 by
the zero-one principle and exercised with structured and random orders up to K = 64, the target's ranks against numpy's
counts with ties, zero weights and NaNs, the independence of voxels, VolumeStitcher.quantiles, interval_figures and
rank_histogram, and --draw_quantiles of the inference script on its four paths.
"""

import ctypes
import importlib.util
import json
import os
import zipfile

import numpy as np
import pytest
import torch

import quantiles_ref as R
from conftest import PKG
from guided_diffusion import _hip, metrics, patches, uncertainty

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
LEVELS = (0, 0.025, 0.25, 0.5, 0.9, 1)
ALL_K = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)      # every template at its full size and one past the previous one


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _weight(n, rng):
    w = (0.25 + rng.random(n)).astype(np.float32)
    w[::7] = 0
    return w


def _order_stats(acc, weight=None):
    """every order statistic s_0 .. s_{K-1} of a (K, n) stack, asked for as (lower = j, frac = 0) in calls of 8"""
    K, n = acc.shape
    a, w = _dev(acc), _dev(weight)
    out = torch.empty((K, n), dtype=torch.float32, device=DEV)
    for j0 in range(0, K, _hip.MAX_QUANTILES):
        nq = min(_hip.MAX_QUANTILES, K - j0)
        _hip.check(_hip.load().ddpm3d_draw_quantiles(
            _hip.ptr(a), _hip.ptr(w), K, n, nq, (ctypes.c_int * nq)(*range(j0, j0 + nq)), (ctypes.c_float * nq)(),
            None, _hip.ptr(out[j0:j0 + nq]), None, None, _hip.stream()))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("K", ALL_K)
def test_quantiles_against_numpy_fp64(K):
    """|out - m| <= 2^-24 (|m| + 2 frac |s_hi - s_lo|) (1 + 2^-20) against m = np.quantile(method="linear") in fp64
    of the fp32 draws: one rounding each of frac, of the difference and of the fma (test_quantiles_cpu.py checks the
    bound against an emulation of the chain).  Where frac == 0 the output is the order statistic itself."""
    rng = np.random.default_rng(100 + K)
    worst = 0.0
    for n in (3 * 4096, 1001):
        for data in ("unit", "offset"):
            for weighted in (False, True):
                x = rng.standard_normal((K, n))
                acc = (x if data == "unit" else 1e4 + 1e-3 * x).astype(np.float32)
                w = _weight(n, rng) if weighted else None
                got = uncertainty.draw_quantiles(_dev(acc), LEVELS, weight=_dev(w)).cpu().numpy().astype(np.float64)
                m = R.quantiles(acc, LEVELS, w)
                lo, hi, frac = R.neighbours(acc, LEVELS, w)
                live = np.ones(n, bool) if w is None else w > 0
                assert np.all(got[:, ~live] == 0)
                bound = 2.0 ** -24 * (np.abs(m) + 2 * frac * np.abs(hi - lo)) * (1 + 2.0 ** -20)
                err = np.abs(got - m)[:, live]
                assert np.all(err <= bound[:, live]), (n, data, weighted, float((err / bound[:, live]).max()))
                worst = max(worst, float((err / np.maximum(bound[:, live], 1e-300)).max()))
                exact = (frac == 0) & live[None]
                assert exact[0].sum() == exact[-1].sum() == live.sum()           # levels 0 and 1 at the least
                assert np.all(got[exact] == lo[exact])
    print("K = %d: largest share of the bound used %.4f" % (K, worst))


# ------------------------------------------------------------------------------------------ 2. the network itself
@pytest.mark.parametrize("K", range(2, 17))
def test_network_sorts_every_zero_one_input(K):
    """All 2^K zero / one inputs as voxels, every order statistic asked for: by the zero-one principle a comparator
    network that sorts these sorts everything, so this proves the networks of KP <= 16 (with their +inf padding)."""
    codes = np.arange(2 ** K, dtype=np.int64)
    acc = ((codes[None] >> np.arange(K)[:, None]) & 1).astype(np.float32)           # (K, 2^K)
    got = _order_stats(acc)
    assert np.array_equal(got, np.sort(acc, axis=0))


def _structured(K):
    up = np.arange(K, dtype=np.float32)
    cols = []
    for r in range(K):
        cols.append(np.roll(up, r))
        cols.append(np.roll(up[::-1], r))
        for split in range(K + 1):                               # two values, every split point, every rotation
            cols.append(np.roll((up >= split).astype(np.float32) * 3 - 1, r))
    return np.stack(cols, axis=1)                                # (K, K (K + 3))


@pytest.mark.parametrize("K", [31, 32, 33, 63, 64])
def test_network_on_structured_and_random_orders(K):
    acc = _structured(K)
    assert np.array_equal(_order_stats(acc), np.sort(acc, axis=0))
    for value in (0.0, -2.5, 1e4 + 1e-3):                         # all equal: every quantile is that value exactly
        flat = np.full((K, 257), value, dtype=np.float32)
        got = uncertainty.draw_quantiles(_dev(flat), LEVELS).cpu().numpy()
        assert np.all(got == np.float32(value))
    rng = np.random.default_rng(K)
    perms = rng.permuted(np.tile(np.arange(K, dtype=np.float32), (100000, 1)), axis=1).T      # (K, 10^5)
    got = _order_stats(perms)
    assert np.array_equal(got, np.broadcast_to(np.arange(K, dtype=np.float32)[:, None], got.shape))


# ------------------------------------------------------------------------------------------ 3. ranks
@pytest.fixture(scope="module", params=[2, 8, 33, 64])
def ranked(request):
    """draws and target in multiples of 1/4 so that ties occur; zero weights, NaN draws and NaN targets sprinkled in"""
    K, n = request.param, 6 * 4096 + 1001
    rng = np.random.default_rng(7 * K)
    acc = (np.round(rng.standard_normal((K, n)) * 4) / 4).astype(np.float32)
    target = (np.round(rng.standard_normal(n) * 4) / 4).astype(np.float32)
    w = np.where(rng.random(n) < 0.5, 1.0, 2.0).astype(np.float32)       # powers of two: the quotients stay on the grid
    w[::7] = 0
    nan_draw = np.zeros(n, bool)
    nan_draw[3::41] = True
    nan_draw &= w > 0
    acc[rng.integers(0, K, n)[nan_draw], np.nonzero(nan_draw)[0]] = np.nan
    nan_target = np.zeros(n, bool)
    nan_target[5::53] = True
    target[nan_target] = np.nan
    quant, below, equal = uncertainty.draw_quantiles(_dev(acc), (0.25, 0.5), weight=_dev(w), target=_dev(target))
    return dict(K=K, n=n, acc=acc, target=target, w=w, nan_draw=nan_draw, nan_target=nan_target, quant=quant,
                below=below, equal=equal)


def test_ranks_equal_numpy_counts(ranked):
    r = ranked
    want_below, want_equal = R.ranks(r["acc"], r["target"], r["w"])
    below, equal = r["below"].cpu().numpy(), r["equal"].cpu().numpy()
    assert below.dtype == equal.dtype == np.uint8
    assert np.array_equal(below, want_below) and np.array_equal(equal, want_equal)
    out = (r["w"] <= 0) | r["nan_draw"] | r["nan_target"]
    assert np.all(below[out] == 255) and np.all(equal[out] == 255) and below[~out].max() <= r["K"]
    assert ((equal > 0) & ~out).sum() > 2000                      # the data really has ties
    quant = r["quant"].cpu().numpy()
    assert np.array_equal(np.isnan(quant), np.broadcast_to(r["nan_draw"], quant.shape)) and r["nan_draw"].sum() > 100
    # the ranks alone: levels=() with a target
    none, b2, e2 = uncertainty.draw_quantiles(_dev(r["acc"]), (), weight=_dev(r["w"]), target=_dev(r["target"]))
    assert none is None and torch.equal(b2, r["below"]) and torch.equal(e2, r["equal"])


def test_rank_histogram_equals_bincount(ranked):
    r = ranked
    below, equal = r["below"].cpu().numpy(), r["equal"].cpu().numpy()
    mask = (np.random.default_rng(1).random(r["n"]) < 0.6).astype(np.uint8)
    for m in (None, mask):
        got = uncertainty.rank_histogram(r["below"], r["equal"], r["K"], mask=_dev(m))
        want = R.rank_histogram(below, equal, r["K"], mask=m)
        assert got == want and len(got["counts"]) == r["K"] + 1
        assert got["n"] == sum(got["counts"]) + got["ties"] and got["ties"] > 0
        counted = (below != 255) if m is None else (below != 255) & (m != 0)
        assert got["n"] == int(counted.sum()) and got["ties"] == int((counted & (equal > 0)).sum())


# ------------------------------------------------------------------------------------------ 4. independence, wrappers
@pytest.mark.parametrize("K", [3, 16, 64])
def test_voxels_are_independent_and_runs_repeat(K):
    n = 2 * 4096 + 2 * 1001
    rng = np.random.default_rng(K)
    acc = rng.standard_normal((K, n)).astype(np.float32)
    w, target = _weight(n, rng), rng.standard_normal(n).astype(np.float32)
    full = uncertainty.draw_quantiles(_dev(acc), LEVELS, weight=_dev(w), target=_dev(target))
    again = uncertainty.draw_quantiles(_dev(acc), LEVELS, weight=_dev(w), target=_dev(target))
    h = n // 2
    half = uncertainty.draw_quantiles(_dev(acc[:, :h]), LEVELS, weight=_dev(w[:h]), target=_dev(target[:h]))
    for a, b, c in zip(full, again, half):
        a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
        bits = (lambda v: v.view(np.uint32)) if a.dtype == np.float32 else (lambda v: v)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a[..., :h]), bits(c))


def test_stitcher_quantiles_are_the_quantiles_of_its_draws():
    shape_dhw, res, K = (20, 40, 37), 16, 5                       # 3 x 3 x 2 patches, cropped along W and Z
    grid = patches.patch_grid(shape_dhw, res)
    rng = np.random.default_rng(3)
    st = uncertainty.VolumeStitcher(shape_dhw, res, K, DEV)
    for i, origin in enumerate(grid):
        st.add(i, _dev(rng.standard_normal((K, 1, res, res, res)).astype(np.float32)), origin)
    target = _dev(rng.standard_normal(st.shape_hwd).astype(np.float32))
    stack = torch.stack([st.draw(k) for k in range(K)])
    quant, below, equal = st.quantiles(LEVELS, target=target)
    want, wb, we = uncertainty.draw_quantiles(stack, LEVELS, target=target)
    assert tuple(quant.shape) == (len(LEVELS), 40, 37, 20)
    assert torch.equal(quant.view(torch.int32), want.view(torch.int32)) and torch.equal(quant, st.quantiles(LEVELS))
    live = st.wsum > 0
    assert 0 < int((~live).sum()) < live.numel()
    assert torch.equal(below[live], wb[live]) and torch.equal(equal[live], we[live])
    assert bool((below[~live] == 255).all()) and bool((equal[~live] == 255).all())
    assert bool((quant[:, ~live] == 0).all())
    only = st.quantiles((), target=target)
    assert only[0] is None and torch.equal(only[1], below) and torch.equal(only[2], equal)
    with pytest.raises(ValueError):
        uncertainty.VolumeStitcher(shape_dhw, res, 1, DEV).quantiles((0.5,))


def test_interval_figures_equal_numpy():
    rng = np.random.default_rng(8)
    shape = (9, 21, 13)
    lo = rng.standard_normal(shape).astype(np.float32)
    hi = lo + rng.random(shape).astype(np.float32)
    t = (lo + 2 * (rng.random(shape).astype(np.float32) - 0.25) * (hi - lo)).astype(np.float32)
    t[::3, ::4] = lo[::3, ::4]                                    # on the bounds: covered
    t[1::3, ::4] = hi[1::3, ::4]
    mask = (rng.random(shape) < 0.7).astype(np.uint8)
    for m in (None, mask):
        got = metrics.interval_figures(_dev(lo), _dev(hi), _dev(t), mask=_dev(m))
        sel = np.ones(shape, bool) if m is None else m != 0
        inside = (lo <= t) & (t <= hi) & sel
        assert got["n_voxels"] == int(sel.sum()) and got["coverage"] == int(inside.sum()) / int(sel.sum())
        assert 0.3 < got["coverage"] < 0.9
        width = (hi.astype(np.float64) - lo.astype(np.float64))[sel].mean()
        assert abs(got["mean_width"] - width) <= 1e-12 * width
    with pytest.raises(ValueError):
        metrics.interval_figures(_dev(lo), _dev(hi), _dev(t), mask=_dev(np.zeros(shape, np.uint8)))


# ------------------------------------------------------------------------------------------ 5. the script
def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(src, save, *extra):
    return _script().main(FLAGS + ["--base_samples", str(src), "--save_dir", str(save)] + list(extra))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("quantiles_script")
    rng = np.random.default_rng(12)
    target = rng.random((20, 24, 24), dtype=np.float32)                            # (D, H, W): 2 x 2 x 2 patches
    vol = (target + 0.1 * rng.standard_normal(target.shape)).astype(np.float32)
    np.savez(d / "pet.npz", vol)
    np.savez(d / "full.npz", target)
    return {"dir": d, "src": d / "pet.npz", "target": d / "full.npz", "target_dhw": target}


PATHS = {"grid": [], "sliding": ["--patch_overlap", "6"], "joint": ["--joint_patches", "True"],
         "regrid": ["--voxel_spacing", "3", "3", "3", "--model_spacing", "2.5", "2.5", "2.5"]}


@pytest.mark.parametrize("path", list(PATHS))
def test_two_draws_min_and_max_give_mean_and_std(files, tmp_path, path):
    """At K = 2 the levels 0 and 1 are the two draws: arr_0 = (q0 + q1) / 2 and std = |q1 - q0| / sqrt(2), an identity
    that needs no second implementation of the draws."""
    out = _run(files["src"], tmp_path / path, "--num_draws", "2", "--draw_quantiles", "0", "1", *PATHS[path])
    with np.load(out) as z:
        assert sorted(z.files) == ["arr_0", "quantile_levels", "quantiles", "std"]
        mean, std, q, levels = z["arr_0"], z["std"], z["quantiles"], z["quantile_levels"]
    assert q.shape == (2,) + mean.shape == (2, 24, 24, 20) and q.dtype == np.float32
    assert levels.dtype == np.float64 and levels.tolist() == [0.0, 1.0]
    q = q.astype(np.float64)
    assert np.all(q[0] <= q[1]) and np.abs(q[1] - q[0]).max() > 0
    assert np.abs((q[0] + q[1]) / 2 - mean).max() <= 2e-6 * np.abs(mean).max()
    assert np.abs(np.abs(q[1] - q[0]) / np.sqrt(2) - std).max() <= 2e-6 * np.abs(std).max()
    assert not os.path.exists(tmp_path / path / "metrics_pet.json")
    assert not [f for f in os.listdir(tmp_path / path) if f.endswith(".tif")]


def test_four_draws_with_a_target(files, tmp_path):
    levels = [0.1, 0.5, 0.9]
    out = _run(files["src"], tmp_path / "o", "--num_draws", "4", "--draw_quantiles", "0.1", "0.5", "0.9",
               "--target_samples", str(files["target"]), "--metrics_mask_threshold", "0.3")
    with np.load(out) as z:
        assert sorted(z.files) == ["arr_0", "quantile_levels", "quantiles", "std"]
        q, std, mean = z["quantiles"], z["std"], z["arr_0"]
        assert z["quantile_levels"].tolist() == levels
    assert q.shape == (3, 24, 24, 20) and q.dtype == np.float32 and np.isfinite(q).all()
    assert np.all(q[0] <= q[1]) and np.all(q[1] <= q[2]) and np.any(q[0] < q[2])
    report = json.load(open(tmp_path / "o" / "metrics_pet.json"))
    row = report["denoised"]
    block = row["quantiles"]
    assert list(block) == ["levels", "rank_histogram", "rank_ties", "rank_n", "interval", "median"]
    # the documented mask: target > threshold * max(target), and a blend weight above 0
    tgt = np.ascontiguousarray(files["target_dhw"].transpose(1, 2, 0))                  # (H, W, Z)
    cover = patches.blend_cover(patches.patch_grid((20, 24, 24), 16), (20, 24, 24), 16)
    mask = (tgt > np.float32(0.3) * tgt.max()) & cover
    n = int(mask.sum())
    assert 0 < n < mask.size and row["n_voxels"] == n
    assert block["levels"] == levels and block["rank_n"] == n and len(block["rank_histogram"]) == 5
    assert sum(block["rank_histogram"]) + block["rank_ties"] == n
    inside = (q[0] <= tgt) & (tgt <= q[2]) & mask
    iv = block["interval"]
    assert list(iv) == ["lower", "upper", "nominal", "coverage", "mean_width"]
    assert iv["lower"] == 0.1 and iv["upper"] == 0.9 and iv["nominal"] == 0.9 - 0.1
    assert iv["coverage"] == int(inside.sum()) / n
    width = (q[2].astype(np.float64) - q[0].astype(np.float64))[mask].mean()
    assert abs(iv["mean_width"] - width) <= 1e-12 * width
    want = metrics.evaluate(_dev(q[1]), _dev(tgt), mask=_dev(mask.astype(np.uint8)), std=_dev(std))
    assert block["median"] == want and list(block["median"]) == [k for k in row if k != "quantiles"]
    log = open(tmp_path / "o" / "log.txt").read()
    assert "interval [q0.1, q0.9]" in log and "nominal 0.8000" in log
    assert "rank histogram of the target among 4 draws" in log and "0.4000 if the target were one more draw" in log


def _members(path):
    with zipfile.ZipFile(path) as z:
        return {n: z.read(n) for n in z.namelist()}


def test_a_run_without_the_flag_is_what_it_was(files, tmp_path):
    out = _run(files["src"], tmp_path / "o", "--num_draws", "2", "--target_samples", str(files["target"]))
    assert set(_members(out)) == {"arr_0.npy", "std.npy"}
    report = json.load(open(tmp_path / "o" / "metrics_pet.json"))
    assert "quantiles" not in report["denoised"] and "quantiles" not in report
    log = open(tmp_path / "o" / "log.txt").read()
    assert "rank histogram" not in log and "interval [" not in log
    # and the flag changes neither arr_0 nor std
    flagged = _run(files["src"], tmp_path / "f", "--num_draws", "2", "--draw_quantiles", "0.5")
    a, b = _members(out), _members(flagged)
    assert a["arr_0.npy"] == b["arr_0.npy"] and a["std.npy"] == b["std.npy"]


def test_two_ranks_write_the_same_bytes_as_one(tmp_path):
    import socket
    import subprocess
    import sys

    rng = np.random.default_rng(9)
    target = rng.random((16, 40, 16), dtype=np.float32)                       # 3 patches of 16^3 along H
    np.savez(tmp_path / "pet.npz", (target + 0.1 * rng.standard_normal(target.shape)).astype(np.float32))
    np.savez(tmp_path / "full.npz", target)
    script = os.path.join(PKG, "scripts", "test.py")
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz"),
                      "--num_draws", "3", "--draw_quantiles", "0.25", "0.5", "1"]
    one = _script().main(common + ["--save_dir", str(tmp_path / "one")])
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), script] + common + [
           "--save_dir", str(tmp_path / "two"), "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = _members(one), _members(tmp_path / "two" / "denoised_pet.npz")
    assert a == b and set(a) == {"arr_0.npy", "std.npy", "quantiles.npy", "quantile_levels.npy"}
    ja = json.load(open(tmp_path / "one" / "metrics_pet.json"))
    jb = json.load(open(tmp_path / "two" / "metrics_pet.json"))
    assert ja == jb and "quantiles" in ja["denoised"]
