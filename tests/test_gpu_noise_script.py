"""
scripts/test.py --device_noise True: the keyed noise on all four paths of the inference script, its
independence of the batch size and of the number of ranks, --noise_seed, and the default path's bytes with the flag
absent (tests/golden/noise_script_default.npz: the script's output before the flag existed).
"""

import importlib.util
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_gpu_script import FLAGS

pytestmark = pytest.mark.gpu

KEYED = ["--device_noise", "True"]


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def volume(tmp_path_factory):
    vol = np.random.default_rng(3).random((20, 40, 40), dtype=np.float32)    # (D, H, W): 3 x 3 x 2 patches of 16^3
    src = tmp_path_factory.mktemp("noise_script") / "pet.npz"
    np.savez(src, vol)
    return src


def _run(src, save, *extra):
    path = _script().main(FLAGS + ["--base_samples", str(src), "--save_dir", str(save)] + list(extra))
    return np.load(path)


@pytest.fixture(scope="module")
def keyed_bs1(volume, tmp_path_factory):
    save = tmp_path_factory.mktemp("keyed_bs1")
    out = _run(volume, save, *KEYED)["arr_0"]
    return out, open(save / "log.txt").read()


def test_keyed_run_does_not_depend_on_the_batch_size(volume, keyed_bs1, tmp_path):
    a, log = keyed_bs1
    assert a.shape == (40, 40, 20) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.abs(a[1:-1, 1:-1, 1:-1]).max() > 0
    assert "Philox4x32-10" in log and "seed 10" in log
    b = _run(volume, tmp_path / "bs4", *KEYED, "--batch_size", "4")["arr_0"]
    # the forwards are not batch-invariant; the noise is (the tolerance of test_gpu_script.py's comparison)
    assert np.abs(a - b).max() < 1e-3 * np.abs(a).max()


def test_noise_seed_gives_another_volume(volume, keyed_bs1, tmp_path):
    a, _ = keyed_bs1
    b = _run(volume, tmp_path / "seed11", *KEYED, "--noise_seed", "11")["arr_0"]
    assert np.isfinite(b).all() and np.abs(a - b).max() > 1e-2 * np.abs(a).max()
    assert "seed 11" in open(tmp_path / "seed11" / "log.txt").read()
    # and the keyed stream is not torch's: another draw than the default path's
    c = _run(volume, tmp_path / "default")["arr_0"]
    assert np.abs(a - c).max() > 1e-2 * np.abs(a).max()


def test_two_rank_keyed_run_equals_one_rank(tmp_path):
    """As test_two_rank_run_equals_one_rank_and_loads_checkpoint: two ranks as a fresh torch.distributed.run child
    (gloo, both on cuda:0), an odd number of patches, the same batch size: equal arrays."""
    vol = np.random.default_rng(9).random((16, 40, 16), dtype=np.float32)   # 3 patches of 16^3 along H
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    common = FLAGS + ["--base_samples", str(src)] + KEYED
    a = np.load(_script().main(common + ["--save_dir", str(tmp_path / "one")]))["arr_0"]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(PKG, "scripts", "test.py")] + common + [
           "--save_dir", str(tmp_path / "two"), "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    b = np.load(tmp_path / "two" / "denoised_pet.npz")["arr_0"]
    assert a.shape == b.shape == (40, 16, 16) and np.abs(a).max() > 0
    assert np.array_equal(a, b)


@pytest.mark.parametrize("extra, has_std", [
    (["--joint_patches", "True"], False), (["--num_draws", "2"], True), (["--patch_overlap", "6"], False),
    (["--joint_patches", "True", "--num_draws", "2", "--patch_overlap", "6"], True)])
def test_keyed_noise_on_the_other_paths(volume, tmp_path, extra, has_std):
    out = _run(volume, tmp_path / "o", *KEYED, *extra)
    arr = out["arr_0"]
    assert arr.shape == (40, 40, 20) and arr.dtype == np.float32 and np.isfinite(arr).all() and np.abs(arr).max() > 0
    assert set(out.files) == ({"arr_0", "std"} if has_std else {"arr_0"})
    if has_std:
        std = out["std"]
        assert std.shape == arr.shape and np.isfinite(std).all() and std.max() > 0


@pytest.mark.parametrize("sampler", [["--use_ddim", "True", "--eta", "0.5"],
                                     ["--use_dpm_solver", "True", "--solver_stochastic", "True"],
                                     ["--use_dpm_solver", "True"]])
def test_keyed_noise_with_the_other_samplers(tmp_path, sampler):
    vol = np.random.default_rng(4).random((16, 16, 16), dtype=np.float32)
    src = tmp_path / "one.npy"
    np.save(src, vol)
    a = _run(src, tmp_path / "a", *KEYED, *sampler)["arr_0"]
    b = _run(src, tmp_path / "b", *KEYED, *sampler, "--noise_seed", "11")["arr_0"]
    assert a.shape == (16, 16, 16) and np.isfinite(a).all() and np.abs(a).max() > 0
    assert not np.array_equal(a, b)


def test_flag_absent_the_output_is_what_it_was(volume, tmp_path):
    """tests/golden/noise_script_default.npz holds the script's output for this volume from the commit before the flag
    existed (same flags, batch sizes 1 and 4, and --num_draws 2 --joint_patches True): the default path's bytes."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "noise_script_default.npz"))
    assert np.array_equal(_run(volume, tmp_path / "bs1")["arr_0"], g["bs1"])
    assert np.array_equal(_run(volume, tmp_path / "off", "--device_noise", "False", "--batch_size", "4")["arr_0"],
                          g["bs4"])
    j = _run(volume, tmp_path / "joint", "--num_draws", "2", "--joint_patches", "True")
    assert np.array_equal(j["arr_0"], g["joint_mean"]) and np.array_equal(j["std"], g["joint_std"])
