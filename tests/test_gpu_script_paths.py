"""
Every path of scripts/test.py against what it wrote before the paths shared one loop and one writer
(tests/golden/script_paths.npz / .json, made by tests/golden/make_script_paths.py from commit 67974df, the last one
with a sampling-and-writing block per path): the same files, the same .npz keys, every array and decoded .tif bit for
bit, and metrics_*.json / trace_*.json equal as parsed (path-valued fields by basename).
"""

import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_script_paths", os.path.join(GOLDEN, "make_script_paths.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def held():
    with np.load(os.path.join(GOLDEN, "script_paths.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "script_paths.json")) as f:
        return arrays, json.load(f)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _check(case, save_dir, held, logs=True):
    arrays, report = held
    files, got, parsed = gen.collect(save_dir)
    keep = lambda names: [n for n in names if logs or not n.startswith("log")]    # every rank keeps a log of its own
    assert keep(files) == keep(report["files"][case])
    want = {k[len(case) + 1:]: v for k, v in arrays.items() if k.startswith(case + "/")}
    assert set(got) == set(want) and want
    for key, w in want.items():
        assert got[key].dtype == w.dtype and got[key].shape == w.shape, key
        assert np.array_equal(_bits(got[key]), _bits(w)), key
    assert parsed == report["json"][case]


@pytest.mark.parametrize("case", list(gen.CASES))
def test_script_path_writes_what_it_wrote(case, tmp_path, held):
    argv = gen.write_inputs(case, str(tmp_path / "in"))
    path = gen.load_script().main(argv + ["--save_dir", str(tmp_path / "out")])
    assert path == str(tmp_path / "out" / "denoised_pet.npz")
    _check(case, str(tmp_path / "out"), held)


def test_two_ranks_write_the_one_rank_files(tmp_path, held):
    """fixed_3q as a fresh two-rank `python -m torch.distributed.run` child (gloo, both ranks on cuda:0): the .npz,
    the metrics file and the trace file are the one-rank fixture's."""
    argv = gen.write_inputs("fixed_3q", str(tmp_path / "in"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(PKG, "scripts", "test.py")] + argv + [
           "--save_dir", str(tmp_path / "out"), "--dist_backend", "gloo", "--share_gpu", "True"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _check("fixed_3q", str(tmp_path / "out"), held, logs=False)
