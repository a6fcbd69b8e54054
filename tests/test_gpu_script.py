"""
End-to-end run of the drop-in inference entry (scripts/test.py): .npz volume ->
tiler -> GPU sampler per sub-volume -> Hann stitcher -> denoised_*.npz.
"""

import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inference_script_npz_end_to_end(tmp_path):
    rng = np.random.default_rng(3)
    vol = rng.random((20, 40, 40), dtype=np.float32)                     # (D, H, W): 3 x 3 x 2 patches of 16^3
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    mod = _script()
    outs = []
    for bs in (1, 4):
        save = tmp_path / ("out_bs%d" % bs)
        path = mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(save), "--batch_size", str(bs)])
        assert path == str(save / "denoised_pet.npz") and os.path.exists(path)
        assert os.path.exists(save / "log.txt")
        arr = np.load(path)["arr_0"]
        assert arr.shape == (40, 40, 20) and arr.dtype == np.float32     # (H, W, Z), key arr_0, like the reference
        assert np.isfinite(arr).all()
        assert np.all(arr[0] == 0) and np.all(arr[:, :, -1] == 0)         # zero-weight Hann border (reference quirk)
        assert np.abs(arr[1:-1, 1:-1, 1:-1]).max() > 0
        outs.append(arr)
    # randomness is keyed per patch: batching 4 patches per forward gives the same volume
    assert np.abs(outs[0] - outs[1]).max() < 1e-3 * np.abs(outs[0]).max()


def test_inference_script_on_the_native_plan_and_step_graph(tmp_path):
    """--native_plan True --step_graph True (the library's own launch plan, replayed as one hipGraph per forward):
    the same stitched volume, bit for bit, as the default launch-by-launch run of the Python plan."""
    vol = np.random.default_rng(5).random((20, 24, 24), dtype=np.float32)
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    mod = _script()
    a = np.load(mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "a")]))["arr_0"]
    b = np.load(mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "b"),
                                  "--native_plan", "True", "--step_graph", "True"]))["arr_0"]
    assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, b)


def test_inference_script_tif_in_tif_out(tmp_path):
    """The reference's own file format (scripts/test.py:96, :169-179, :192): a (Z, H, W) .tif stack in, denoised_<name>.npz
    (H, W, Z) AND denoised_<name>.tif (Z, H, W, float32) out; uint16 samples as scanners write them."""
    from guided_diffusion import tiff_io
    vol = (np.random.default_rng(6).random((20, 24, 24)) * 4000).astype(np.uint16)
    src = tmp_path / "pet.tif"
    tiff_io.imwrite(str(src), vol)
    mod = _script()
    path = mod.main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o")])
    assert path == str(tmp_path / "o" / "denoised_pet.npz")
    arr = np.load(path)["arr_0"]
    tif = tiff_io.imread(str(tmp_path / "o" / "denoised_pet.tif"))
    assert arr.shape == (24, 24, 20) and tif.shape == (20, 24, 24) and tif.dtype == np.float32
    assert np.array_equal(tif, arr.transpose(2, 0, 1).astype(np.float32)) and np.isfinite(tif).all() and np.abs(tif).max() > 0
    # the same volume handed over as .npz gives the same result: the loader, not the format, defines the input
    np.savez(tmp_path / "pet2.npz", vol.astype(np.float32))
    again = np.load(mod.main(FLAGS + ["--base_samples", str(tmp_path / "pet2.npz"), "--save_dir", str(tmp_path / "p")]))["arr_0"]
    assert np.array_equal(arr, again)


def test_inference_script_ddim_and_fp16_flags(tmp_path):
    vol = np.random.default_rng(4).random((16, 16, 16), dtype=np.float32)
    src = tmp_path / "one.npy"
    np.save(src, vol)
    mod = _script()
    flags = [f if f != "3" else "ddim3" for f in FLAGS]
    path = mod.main(flags + ["--base_samples", str(src), "--save_dir", str(tmp_path / "o"), "--use_ddim", "True",
                             "--use_fp16", "True"])
    arr = np.load(path)["arr_0"]
    assert arr.shape == (16, 16, 16) and np.isfinite(arr).all()


def test_two_rank_run_equals_one_rank_and_loads_checkpoint(tmp_path):
    """The reference's launch shape (test_DDPM_3d_mpi.sh: N ranks, patch i -> rank i mod N, all_gather
    of finished patches, scripts/test.py:74-78, 235-246) rehearsed with TWO ranks as a fresh
    `python -m torch.distributed.run` child (gloo, both ranks on cuda:0 -- no multi-GPU node here):
    an odd number of patches (the uneven work list the reference hangs on), weights read from a
    --model_path checkpoint by every rank (dist_util.load_state_dict, dist_util.py:58-78).  The
    stitched volume must equal the single-process run bit for bit: noise is keyed by the global
    patch index and every kernel is deterministic."""
    import socket
    import subprocess
    import sys

    import torch
    from guided_diffusion import script_util as su
    from guided_diffusion import synth

    fl = su.sr_model_and_diffusion_defaults()
    fl.update(large_size=16, small_size=16, num_channels=32, num_res_blocks=1, num_head_channels=64,
              attention_resolutions="1000", learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True)
    model, _ = su.sr_create_model_and_diffusion(**fl)
    sd = {k: torch.from_numpy(synth.synth_param(k, tuple(v.shape), 5)) for k, v in model.state_dict().items()}
    ckpt = tmp_path / "model.pt"
    torch.save(sd, ckpt)

    vol = np.random.default_rng(9).random((16, 40, 16), dtype=np.float32)   # 3 patches of 16^3 along H
    src = tmp_path / "pet.npz"
    np.savez(src, vol)
    script = os.path.join(PKG, "scripts", "test.py")
    common = FLAGS + ["--base_samples", str(src), "--model_path", str(ckpt)]

    one = _script().main(common + ["--save_dir", str(tmp_path / "one")])
    a = np.load(one)["arr_0"]

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), script] + common + [
           "--save_dir", str(tmp_path / "two"), "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    b = np.load(tmp_path / "two" / "denoised_pet.npz")["arr_0"]
    assert a.shape == b.shape == (40, 16, 16)
    assert np.array_equal(a, b)
    assert np.abs(a).max() > 0
    # synthetic-seed weights (no --model_path) are different weights: the checkpoint was really used
    c = np.load(_script().main(FLAGS + ["--base_samples", str(src), "--save_dir", str(tmp_path / "syn")]))["arr_0"]
    assert not np.array_equal(a, c)


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher around it (the reference's launcher is
    one command, test_DDPM_3d_mpi.sh:5): the parent starts a two-rank torch.distributed.run child,
    relays rank 0's ONE JSON line and its exit status.  Rehearsal on the one-GPU box: gloo, both ranks
    on cuda:0, tiny network, 5 DDPM steps."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--dist-backend", "gloo",
           "--steps", "1", "--warmup", "0", "--ddpm-steps", "5", "--arch", "tiny", "--size", "16",
           "--cpu-steps", "0", "--probe-ms", "5", "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak"
    # the collective library that ran is named: this rehearsal is gloo, so the line claims no RCCL ranks
    assert rec["collective_ranks"] == 2 and rec["collective_backend"] == "gloo" and rec["rccl_ranks"] is None
    assert rec["steps"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    # --dump-outputs: the last timed step's samples as rank 0 received them, both ranks in rank order
    out = np.load(tmp_path / "dump" / "sample.npy")
    assert out.dtype == np.float32 and out.shape == (2, 1, 16, 16, 16) and np.isfinite(out).all()
    assert not np.array_equal(out[0], out[1])                            # each rank sampled its own volume
    # a launcher that hands over the wrong world size is refused, not silently accepted
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--steps", "1"],
                         env=dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"), capture_output=True, text=True,
                         timeout=600)
    assert bad.returncode != 0 and "WORLD_SIZE" in bad.stderr


def test_bench_plain_run_is_lean_and_full_adds_the_rest(tmp_path):
    """A plain `bench.py` run times its steps and prints the headline with the roofline of those steps only;
    `--full` adds what takes runs of its own (MFMA calibration, exact_f32, parity, cpu_baseline) after the
    timed region and leaves the headline fields and the dumped samples as they are.  Tiny network, 16^3."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    common = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--ddpm-steps", "5",
              "--arch", "tiny", "--size", "16", "--cpu-steps", "1", "--probe-ms", "5"]
    recs = {}
    for name, extra in (("plain", []), ("full", ["--full"])):
        r = subprocess.run(common + extra + ["--dump-outputs", str(tmp_path / name)], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        recs[name] = json.loads(lines[0])
    plain, full = recs["plain"], recs["full"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus", "config"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["full"] is False and full["full"] is True
    # plain: the timed steps' own roofline, nothing that needs another run
    assert plain["roofline"]["launches_timed"] > 0 and "device_sustained_tflops" not in plain["roofline"]
    assert plain["exact_f32"] is None and plain["parity"] is None and plain["cpu_baseline"] is None
    # --full: all of it, as before the option existed
    assert full["roofline"]["device_sustained_tflops"] > 0 and full["roofline"]["frac_of_sustained"] > 0
    assert full["exact_f32"]["steps_timed"] == 5
    assert set(full["parity"]) == {"vs_exact_f32", "vs_cpu_oracle"}
    assert full["parity"]["vs_exact_f32"]["rel_err"] < 1e-3 and full["parity"]["vs_cpu_oracle"]["rel_err"] < 1e-3
    assert full["cpu_baseline"]["value"] > 0
    # the timed steps are the same in both: same seeded inputs, same samples
    a, b = np.load(tmp_path / "plain" / "sample.npy"), np.load(tmp_path / "full" / "sample.npy")
    assert a.shape == (1, 1, 16, 16, 16) and np.isfinite(a).all()
    assert np.array_equal(a, b)


def test_c_abi_from_plain_cpp(tmp_path):
    """The boundary is a C ABI, not a Python extension: tests/c_abi/conv_from_c.cpp (no Python, no torch:
    hipMalloc'd buffers, `ddpm3d.h`, -lddpm3d) packs weights and runs one fused conv in the exact and the
    f16x3 arithmetic, checks output and GroupNorm partial sums against a scalar host loop and the error
    reporting path.  Compiled here with hipcc and run as a child process."""
    import shutil
    import subprocess
    from conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    csrc = os.path.join(PKG, "csrc")
    exe = str(tmp_path / "conv_from_c")
    cmd = [hipcc, "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "conv_from_c.cpp"),
           "-L", csrc, "-lddpm3d", "-Wl,-rpath," + csrc, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "C ABI OK" in r.stdout


def test_whole_network_from_plain_cpp(tmp_path):
    """SURVEY 8b's `unet_forward(handle, ...)` granularity from a host that is neither Python nor torch:
    tests/c_abi/unet_from_c.cpp describes a small FiLM-conditioned SuperRes UNet (encoder, middle and decoder
    ResBlocks, the decoder's virtual concat with 1x1 skip convs) with ddpm3d_unet_desc, has the library compile
    the launch plan into one hipMalloc'ed arena (ddpm3d_unet_plan_create), runs ddpm3d_unet_forward twice
    (bit-identical replays) and checks the output against its own fp64 evaluation of the network on the host;
    an undersized arena is refused."""
    import shutil
    import subprocess
    from conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    csrc = os.path.join(PKG, "csrc")
    exe = str(tmp_path / "unet_from_c")
    cmd = [hipcc, "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "unet_from_c.cpp"),
           "-L", csrc, "-lddpm3d", "-Wl,-rpath," + csrc, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "PASS" in r.stdout and "bit-identical" in r.stdout
