"""
CPU tier of the variational-bound entry points (calc_bpd_loop and its helpers): the C ABI declares and exports
them, sizes their workspace, refuses bad arguments on the host before any HIP call, and the forward-process
table they read is the reference's fp64 schedule rounded once.  No GPU is touched here.
"""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from guided_diffusion import _hip
from guided_diffusion import script_util as su

NEW = ["ddpm3d_q_sample", "ddpm3d_vb_terms_workspace_bytes", "ddpm3d_vb_terms", "ddpm3d_prior_bpd"]
FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _hip.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert re.search(r"DDPM3D_NQCOEF = 4\b", hdr) and _hip.NQCOEF == 4


def test_workspace_bytes():
    """One 32-byte record per (sample, slice of 1024 elements), at most 1024 slices per sample."""
    lib = _hip.load()
    ws = lib.ddpm3d_vb_terms_workspace_bytes
    assert ws(1, 64 ** 3) == 256 * 32
    assert ws(3, 16 * 32 * 32) == 3 * 16 * 32
    assert ws(2, 1) == 2 * 32
    assert ws(1, 1025) == 2 * 32
    assert ws(1, 1024 * 1024) == 1024 * 32
    assert ws(2, 128 ** 3) == 2 * 1024 * 32            # capped: each slice then walks more than 1024 elements
    assert ws(0, 100) == 0 and ws(1, 0) == 0 and ws(-1, 5) == 0


def _vb_args(**over):
    a = dict(model_out=FAKE, x_start=FAKE, x_t=FAKE, noise=FAKE, coef=FAKE, qcoef=FAKE, t_idx=FAKE, N=2,
             voxels=4096, T=10, flags=_hip.F_LEARN_SIGMA | _hip.F_CLIP, ws=FAKE, ws_bytes=2 * 4 * 32, vb=FAKE,
             xstart_mse=FAKE, mse=FAKE, ld_out=10, pred_xstart=None, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over", [
    dict(model_out=None), dict(x_start=None), dict(x_t=None), dict(coef=None), dict(qcoef=None), dict(t_idx=None),
    dict(vb=None), dict(noise=None), dict(mse=None), dict(ws=None),
    dict(N=0), dict(N=-1), dict(N=65536), dict(voxels=0), dict(voxels=-5), dict(T=0), dict(T=-1),
    dict(ld_out=0), dict(flags=8), dict(ws_bytes=2 * 4 * 32 - 1), dict(ws=FAKE + 8),
])
def test_vb_terms_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_vb_terms(*_vb_args(**over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("vb_terms:")


@pytest.mark.parametrize("over", [
    dict(x_start=None), dict(noise=None), dict(qcoef=None), dict(t_idx=None), dict(x_t=None),
    dict(N=0), dict(N=65536), dict(voxels=0), dict(T=0),
])
def test_q_sample_refuses_bad_arguments(over):
    a = dict(x_start=FAKE, noise=FAKE, qcoef=FAKE, t_idx=FAKE, N=1, voxels=64, T=10, x_t=FAKE, stream=None)
    a.update(over)
    lib = _hip.load()
    assert lib.ddpm3d_q_sample(*a.values()) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("q_sample:")


@pytest.mark.parametrize("over", [
    dict(x_start=None), dict(qcoef=None), dict(out=None), dict(ws=None), dict(N=0), dict(voxels=0), dict(T=0),
    dict(ws_bytes=31), dict(ws=FAKE + 4),
])
def test_prior_bpd_refuses_bad_arguments(over):
    a = dict(x_start=FAKE, qcoef=FAKE, N=1, voxels=64, T=10, ws=FAKE, ws_bytes=32, out=FAKE, stream=None)
    a.update(over)
    lib = _hip.load()
    assert lib.ddpm3d_prior_bpd(*a.values()) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("prior_bpd:")


@pytest.mark.parametrize("tag,resp", [("full", ""), ("250", "250"), ("50", "50"), ("10", "10")])
@pytest.mark.parametrize("learn_sigma", [True, False])
def test_qcoef_table_is_the_fp64_schedule_rounded_once(tag, resp, learn_sigma):
    """The four columns against the reference's own fp64 tables (schedules.npz), bit for bit after one rounding.
    The posterior log-variance column does not depend on the variance type (FIXED_LARGE included)."""
    g = np.load(os.path.join(GOLDEN, "schedules.npz"))
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=learn_sigma, timestep_respacing=resp)
    tab = d.qcoef_table()
    assert tab.dtype == np.float32 and tab.shape == (d.num_timesteps, _hip.NQCOEF)
    for col, name in enumerate(["sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                                "log_one_minus_alphas_cumprod", "posterior_log_variance_clipped"]):
        assert np.array_equal(tab[:, col], g[tag + "/" + name].astype(np.float32)), (tag, name)
