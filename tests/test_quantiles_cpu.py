"""
CPU tier of the posterior quantile maps and the rank calibration: quantile_positions reproduces
numpy.quantile's "linear" positions for every K, ddpm3d_draw_quantiles is declared, exported and bound within ABI 13 and
refuses every bad argument on the host before any HIP call, and the inference script refuses a bad --draw_quantiles
before it builds a model.  The error bound the GPU tests hold the interpolation to is checked here against a numpy
emulation of the kernel's fp32 chain.  No GPU is touched.
"""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT
from guided_diffusion import _hip, uncertainty

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
LEVELS = (0, 0.025, 0.1, 0.25, 0.5, 0.75, 0.9, 0.975, 1)


@pytest.mark.parametrize("K", range(2, 65))
def test_positions_reproduce_numpy(K):
    draws = np.arange(K, dtype=np.float64)
    for group in (LEVELS[:8], LEVELS[1:], LEVELS[4:5]):
        lower, frac = uncertainty.quantile_positions(group, K)
        assert len(lower) == len(frac) == len(group)
        for q, lo, f in zip(group, lower, frac):
            assert isinstance(lo, int) and 0 <= lo <= K - 1 and 0.0 <= f < 1.0
            assert lo < K - 1 or f == 0.0
            assert abs(lo + f - np.quantile(draws, q, method="linear")) <= 1e-12


@pytest.mark.parametrize("levels,K", [
    ((), 4), (tuple(i / 8 for i in range(9)), 16),              # none, nine
    ((-0.1, 0.5), 4), ((0.5, 1.5), 4), ((float("nan"),), 4),    # outside [0, 1]
    ((0.5, 0.5), 4), ((0.9, 0.1), 4),                           # not strictly ascending
    ((0.5,), 1), ((0.5,), 65), ((0.5,), 4.0),                   # K outside 2..64, or no int
])
def test_positions_refuse(levels, K):
    with pytest.raises(ValueError):
        uncertainty.quantile_positions(levels, K)


def test_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    name = "ddpm3d_draw_quantiles"
    assert name in declared and name in _hip.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define DDPM3D_MAX_QUANTILES %d\b" % _hip.MAX_QUANTILES, hdr) and _hip.MAX_QUANTILES == 8
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13


def _args(**over):
    a = dict(acc=FAKE, wsum=FAKE, K=8, voxels=4096, nq=2, lower=[1, 6], frac=[0.25, 0.5], target=FAKE, quant=FAKE,
             below=FAKE, equal=FAKE, stream=None)
    a.update(over)
    for key, ctype in (("lower", ctypes.c_int), ("frac", ctypes.c_float)):
        if a[key] is not None:
            a[key] = (ctype * max(len(a[key]), 1))(*a[key])
    return list(a.values())


NO_TARGET = dict(target=None, below=None, equal=None)


@pytest.mark.parametrize("over", [
    dict(acc=None),
    dict(K=1), dict(K=65),
    dict(voxels=0),
    dict(nq=-1), dict(nq=9, lower=[0] * 9, frac=[0.0] * 9),
    dict(nq=0, **NO_TARGET),
    dict(quant=None),
    dict(lower=[-1, 6]), dict(lower=[1, 8]),
    dict(frac=[0.25, float("nan")]), dict(frac=[0.25, float("inf")]), dict(frac=[-0.25, 0.5]), dict(frac=[0.25, 1.0]),
    dict(lower=[1, 7]),                                          # the last draw with frac 0.5
    dict(target=None), dict(below=None), dict(equal=None), dict(target=None, below=None),
])
def test_entry_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_draw_quantiles(*_args(**over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("draw_quantiles:")


def test_fp32_chain_stays_within_the_bound():
    """|out - m| <= 2^-24 (|m| + 2 frac |s_hi - s_lo|) (1 + 2^-20): one rounding each of frac (relative 2^-24 on
    frac * delta), of the difference (another 2^-24 on frac * delta) and of the fma's result (2^-24 |m|, to first order).
    A numpy emulation of the kernel's chain (fp32 frac, fp32 difference, the fma as an fp64 product and sum rounded
    once: exact for these magnitudes up to a double rounding far below 2^-20) stays within it on 200 000 voxels."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for K in (2, 5, 8, 17, 64):
        for data in (rng.standard_normal((K, 200000)).astype(np.float32),
                     (1e4 + 1e-3 * rng.standard_normal((K, 200000))).astype(np.float32)):
            s = np.sort(data, axis=0)
            for q in (0.025, 0.25, 0.9):
                (j,), (f,) = uncertainty.quantile_positions((q,), K)
                lo, hi = s[j].astype(np.float64), s[j + 1].astype(np.float64)
                m = lo + f * (hi - lo)
                d32 = (s[j + 1] - s[j]).astype(np.float64)
                got = (np.float64(np.float32(f)) * d32 + lo).astype(np.float32).astype(np.float64)
                bound = 2.0 ** -24 * (np.abs(m) + 2 * f * np.abs(hi - lo)) * (1 + 2.0 ** -20)
                assert np.all(np.abs(got - m) <= bound)
                worst = max(worst, float((np.abs(got - m) / bound).max()))
    print("largest share of the bound used: %.4f" % worst)
    assert 0.5 < worst <= 1.0


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("flags", [
    ["--draw_quantiles", "0.1", "0.9"],                                                    # without --num_draws >= 2
    ["--num_draws", "4", "--draw_quantiles"] + [str(i / 10) for i in range(9)],            # nine levels
    ["--num_draws", "4", "--draw_quantiles", "0.5", "1.5"],                                # outside [0, 1]
    ["--num_draws", "4", "--draw_quantiles", "0.5", "0.5"],                                # not strictly ascending
])
def test_script_refuses_bad_quantiles_before_building_a_model(flags, tmp_path, monkeypatch):
    mod = _script()

    def no_model(*a, **kw):
        raise AssertionError("a model was built")

    monkeypatch.setattr(mod, "sr_create_model_and_diffusion", no_model)
    monkeypatch.setattr(mod.dist_util, "setup_dist", no_model)
    with pytest.raises(SystemExit) as e:
        mod.main(flags + ["--base_samples", str(tmp_path / "none.npz"), "--save_dir", str(tmp_path)])
    assert e.value.code == 2


def test_script_defaults_to_no_quantiles():
    assert _script().create_argparser().parse_args([]).draw_quantiles is None
