"""
scripts/test.py --consistency_fwhm: the low-pass data-consistency guidance on all four paths of the
inference script and its three samplers, the "consistency" block of metrics_<name>.json, weight 0 as a report-only run,
--model_spacing's effective spacing, and the independence of the number of ranks.  Phantom and settings of
tests/test_gpu_noise_script.py.  The flags' refusals are checked without a GPU in tests/test_guidance_cpu.py.
"""

import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from guided_diffusion import guidance
from test_gpu_script import FLAGS

pytestmark = pytest.mark.gpu

ON = ["--consistency_fwhm", "8", "--voxel_spacing", "2", "2", "2"]
KEYS = {"fwhm_mm", "sigma_voxels", "radii", "weight", "stop_t", "lowpass_rms"}


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def volume(tmp_path_factory):
    vol = np.random.default_rng(3).random((20, 40, 40), dtype=np.float32)    # (D, H, W): 3 x 3 x 2 patches of 16^3
    src = tmp_path_factory.mktemp("guidance_script") / "pet.npz"
    np.savez(src, vol)
    return src


def _run(src, save, *extra):
    """-> (the .npz, its bytes, the "consistency" block or None, the log)"""
    path = _script().main(FLAGS + ["--base_samples", str(src), "--save_dir", str(save)] + list(extra))
    mpath = os.path.join(os.path.dirname(path), "metrics_pet.json")
    block = None
    if os.path.exists(mpath):
        report = json.load(open(mpath))
        assert set(report) == {"consistency"}            # no target: the block is the whole file
        block = report["consistency"]
    return np.load(path), open(path, "rb").read(), block, open(os.path.join(str(save), "log.txt")).read()


@pytest.fixture(scope="module")
def guided(volume, tmp_path_factory):
    return _run(volume, tmp_path_factory.mktemp("guided"), *ON)


def test_weight_zero_only_reports_and_weight_one_pulls(volume, guided, tmp_path):
    plain, plain_bytes, none, plain_log = _run(volume, tmp_path / "plain")
    assert none is None and "consistency" not in plain_log
    off, off_bytes, b0, log0 = _run(volume, tmp_path / "w0", *ON, "--consistency_weight", "0")
    assert off_bytes == plain_bytes                     # the .npz, byte for byte
    out, _, b1, log1 = guided
    arr = out["arr_0"]
    assert arr.shape == (40, 40, 20) and arr.dtype == np.float32 and np.isfinite(arr).all()
    assert not np.array_equal(arr, plain["arr_0"])
    ref = guidance.LowPassPull(8.0, (2.0, 2.0, 2.0))
    for b, w in ((b0, 0.0), (b1, 1.0)):
        assert set(b) == KEYS and b["fwhm_mm"] == 8.0 and b["radii"] == [5, 5, 5] and b["weight"] == w
        assert b["stop_t"] == 0 and b["sigma_voxels"] == list(ref.taps.sigma_voxels) and b["lowpass_rms"] > 0
    print("lowpass_rms at weight 0: %.6g, at weight 1: %.6g" % (b0["lowpass_rms"], b1["lowpass_rms"]))
    assert b1["lowpass_rms"] < b0["lowpass_rms"]
    for log in (log0, log1):
        assert log.count("consistency guidance: FWHM 8 mm") == 1
    assert "only reports" in log0 and "only reports" not in log1


@pytest.mark.parametrize("extra, has_std", [
    (["--num_draws", "2"], True), (["--patch_overlap", "6", "--device_noise", "True"], False),
    (["--joint_patches", "True"], False),
    (["--joint_patches", "True", "--num_draws", "2", "--patch_overlap", "6", "--device_noise", "True"], True)])
def test_guidance_on_the_other_paths(volume, guided, tmp_path, extra, has_std):
    out, _, block, _ = _run(volume, tmp_path / "o", *ON, *extra)
    arr = out["arr_0"]
    assert arr.shape == (40, 40, 20) and arr.dtype == np.float32 and np.isfinite(arr).all() and np.abs(arr).max() > 0
    assert set(out.files) == ({"arr_0", "std"} if has_std else {"arr_0"})
    assert set(block) == KEYS and block["lowpass_rms"] > 0
    un = _run(volume, tmp_path / "u", *ON, "--consistency_weight", "0", *extra)[2]
    assert block["lowpass_rms"] < un["lowpass_rms"]


@pytest.mark.parametrize("sampler", [["--use_ddim", "True", "--eta", "0.5"],
                                     ["--use_dpm_solver", "True", "--solver_stochastic", "True"],
                                     ["--use_dpm_solver", "True"]])
def test_guidance_with_the_other_samplers(tmp_path, sampler):
    vol = np.random.default_rng(4).random((16, 16, 16), dtype=np.float32)
    src = tmp_path / "pet.npy"
    np.save(src, vol)
    a, _, ba, _ = _run(src, tmp_path / "a", *sampler, "--consistency_fwhm", "0", "--consistency_stop_t", "400")
    b, _, bb, _ = _run(src, tmp_path / "b", *sampler, "--consistency_fwhm", "0", "--consistency_weight", "0")
    assert a["arr_0"].shape == (16, 16, 16) and np.isfinite(a["arr_0"]).all()
    assert not np.array_equal(a["arr_0"], b["arr_0"])
    assert ba["radii"] == [0, 0, 0] and ba["stop_t"] == 400 and ba["lowpass_rms"] < bb["lowpass_rms"]


def test_model_spacing_builds_the_taps_at_the_effective_spacing(tmp_path):
    vol = np.random.default_rng(5).random((16, 24, 24), dtype=np.float32)
    src = tmp_path / "pet.npy"
    np.save(src, vol)
    path = _script().main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o"), "--consistency_fwhm",
                                   "8", "--voxel_spacing", "2", "2", "2", "--model_spacing", "2", "3", "3"])
    assert np.isfinite(np.load(path)["arr_0"]).all()
    block = json.load(open(tmp_path / "o" / "metrics_pet.json"))["consistency"]
    assert block["radii"] == list(guidance.LowPassPull(8.0, (2.0, 3.0, 3.0)).radii) == [5, 3, 3]


def test_two_rank_guided_run_equals_one_rank(tmp_path):
    vol = np.random.default_rng(9).random((16, 40, 16), dtype=np.float32)   # 3 patches of 16^3 along H
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    common = FLAGS + ["--base_samples", str(src)] + ON
    one = _script().main(common + ["--save_dir", str(tmp_path / "one")])
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(PKG, "scripts", "test.py")] + common + [
           "--save_dir", str(tmp_path / "two"), "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    two = tmp_path / "two" / "denoised_pet.npz"
    assert open(one, "rb").read() == open(two, "rb").read()
    assert json.load(open(tmp_path / "one" / "metrics_pet.json")) == json.load(open(tmp_path / "two" / "metrics_pet.json"))
