"""
CPU tier of p_mean_variance and DDIM inversion (ddim_reverse_sample and its loop): the C ABI declares and exports
both entries, refuses bad arguments on the host before any HIP call, and the Python layer refuses what it does not
run (eta != 0, denoised_fn, host tensors) before the model is called.  No GPU is touched here.
"""

import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT
from guided_diffusion import _hip
from guided_diffusion import script_util as su

NEW = ["ddpm3d_p_mean_variance", "ddpm3d_ddim_reverse_step"]
FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _hip.EXPORTS, name
        assert hasattr(lib, name), name
    # entries added within ABI 13: the number does not move
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13


def _pmv_args(**over):
    a = dict(model_out=FAKE, x=FAKE, coef=FAKE, t_idx=FAKE, N=2, voxels=4096, T=10,
             flags=_hip.F_LEARN_SIGMA | _hip.F_CLIP, mean=FAKE, variance=FAKE, log_variance=FAKE, pred_xstart=FAKE,
             stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over", [
    dict(model_out=None), dict(x=None), dict(coef=None), dict(t_idx=None), dict(mean=None), dict(pred_xstart=None),
    dict(N=0), dict(N=-1), dict(N=65536), dict(voxels=0), dict(voxels=-5), dict(T=0), dict(T=-1),
    dict(flags=8), dict(flags=_hip.F_CLIP | 16),
    dict(variance=None), dict(log_variance=None), dict(variance=None, log_variance=None),
    dict(flags=_hip.F_CLIP), dict(flags=0, variance=None), dict(flags=_hip.F_PREDICT_XSTART, log_variance=None),
])
def test_p_mean_variance_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_p_mean_variance(*_pmv_args(**over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("p_mean_variance:")


@pytest.mark.parametrize("over", [
    dict(model_out=None), dict(x=None), dict(coef=None), dict(t_idx=None), dict(sample=None),
    dict(N=0), dict(N=-1), dict(N=65536), dict(voxels=0), dict(voxels=-5), dict(T=0), dict(T=-1),
    dict(flags=8), dict(flags=-1),
])
def test_ddim_reverse_step_refuses_bad_arguments(over):
    a = dict(model_out=FAKE, x=FAKE, coef=FAKE, t_idx=FAKE, N=1, voxels=64, T=10, flags=_hip.F_LEARN_SIGMA,
             sample=FAKE, pred_xstart=None, stream=None)
    a.update(over)
    lib = _hip.load()
    assert lib.ddpm3d_ddim_reverse_step(*a.values()) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("ddim_reverse_step:")


class _Model:
    """Records calls; any call is a failure of the tests below."""

    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("the model must not be called")

    def parameters(self):
        return iter([torch.zeros(1)])


def _setup():
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing="ddim10")
    x = torch.zeros((1, 1, 4, 8, 8))
    return d, _Model(), x, torch.tensor([3])


def test_nonzero_eta_is_refused_before_the_model_runs():
    d, m, x, t = _setup()
    with pytest.raises(AssertionError, match="deterministic"):
        d.ddim_reverse_sample(m, x, t, eta=0.5)
    with pytest.raises(AssertionError, match="deterministic"):
        d.ddim_reverse_sample_loop(m, x, eta=1.0)
    with pytest.raises(AssertionError, match="deterministic"):
        next(d.ddim_reverse_sample_loop_progressive(m, x, eta=-0.1))
    assert m.calls == 0


def test_nonzero_eta_is_refused_under_python_O():
    """The reference's `assert eta == 0.0` is raised explicitly: `python -O` does not strip it."""
    code = ("import torch\nfrom guided_diffusion import script_util as su\n"
            "d = su.create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing='10')\n"
            "try:\n    d.ddim_reverse_sample(None, torch.zeros(1, 1, 2, 2, 2), torch.tensor([0]), eta=0.5)\n"
            "except AssertionError:\n    print('refused')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run([sys.executable, "-O", "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:]


def test_denoised_fn_is_refused_before_the_model_runs():
    d, m, x, t = _setup()
    fn = lambda v: v  # noqa: E731
    with pytest.raises(NotImplementedError):
        d.ddim_reverse_sample(m, x, t, denoised_fn=fn)
    with pytest.raises(NotImplementedError):
        d.p_mean_variance(m, x, t, denoised_fn=fn)
    with pytest.raises(NotImplementedError):
        d.ddim_reverse_sample_loop(m, x, denoised_fn=fn)
    assert m.calls == 0


def test_cpu_tensors_are_refused_before_the_model_runs():
    d, m, x, t = _setup()
    with pytest.raises(RuntimeError, match="GPU"):
        d.ddim_reverse_sample(m, x, t)
    with pytest.raises(RuntimeError, match="GPU"):
        d.p_mean_variance(m, x, t)
    with pytest.raises(RuntimeError, match="GPU"):
        d.ddim_reverse_sample_loop(m, x)
    with pytest.raises(RuntimeError, match="GPU"):
        d.ddim_reverse_sample_loop(m, x, device="cpu")
    assert m.calls == 0
