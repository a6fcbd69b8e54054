"""
CPU tier of the per-voxel uncertainty maps (mean and sample std of K posterior draws): the two C entries are
declared, exported and bound within ABI 13 and refuse bad arguments on the host before any HIP call; the per-draw
generators keep draw 0 on the single-draw stream and give every (patch, draw) a stream of its own that does not
depend on K; the inference script refuses --num_draws below 1 before it builds a model.  No GPU is touched here.
"""

import ctypes
import importlib.util
import os
import re

import pytest
import torch

from conftest import PKG, ROOT
from guided_diffusion import _hip, dist_util

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_draw_stitch", "ddpm3d_draw_moments")


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_MAX_DRAWS %d\b" % _hip.MAX_DRAWS, hdr)
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13


def _stitch_args(**over):
    a = dict(samples=FAKE, K=3, res=16, window=FAKE, xs=0, ys=4, zs=2, H=40, W=37, D=20, acc=FAKE, wsum=FAKE,
             stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over", [
    dict(samples=None), dict(window=None), dict(acc=None), dict(wsum=None),
    dict(K=0), dict(K=-1), dict(K=65),
    dict(res=0), dict(res=-16), dict(res=1025), dict(H=0), dict(W=-1), dict(D=0),
    dict(xs=-1), dict(ys=-1), dict(zs=-1), dict(xs=40), dict(ys=37), dict(zs=20), dict(xs=1000, ys=1000),
])
def test_draw_stitch_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_draw_stitch(*_stitch_args(**over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("draw_stitch:")


def _moments_args(**over):
    a = dict(acc=FAKE, wsum=FAKE, K=4, voxels=4096, mean=FAKE, std=FAKE, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over", [
    dict(acc=None), dict(mean=None), dict(std=None), dict(acc=None, wsum=None),
    dict(K=1), dict(K=0), dict(K=-3), dict(K=65),
    dict(voxels=0), dict(voxels=-1), dict(voxels=1 << 60),
])
def test_draw_moments_refuses_bad_arguments(over):
    lib = _hip.load()
    assert lib.ddpm3d_draw_moments(*_moments_args(**over)) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode().startswith("draw_moments:")


def _stream(g, n=64):
    return torch.randn(n, generator=g, device="cpu")


def test_draw_zero_is_the_single_draw_stream():
    for i in (0, 1, 17, 1000002):
        today = torch.Generator(device="cpu")
        today.manual_seed(10 * 1000003 + i)                       # the seed volume_generator(i) has always used
        want = _stream(today)
        assert torch.equal(_stream(dist_util.volume_generator(i, device="cpu", draw=0)), want)
        assert torch.equal(_stream(dist_util.volume_generator(i, device="cpu")), want)


def test_draw_streams_differ_and_do_not_depend_on_k():
    streams = {}
    for i in range(3):
        for d in range(4):
            streams[(i, d)] = _stream(dist_util.volume_generator(i, device="cpu", draw=d))
    keys = list(streams)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            assert not torch.equal(streams[keys[a]], streams[keys[b]]), (keys[a], keys[b])
    # the generator of (patch, draw) is a function of those two alone: asking for it again -- as a run with another
    # K, batch size or world size does -- gives the same stream
    for (i, d), s in streams.items():
        assert torch.equal(_stream(dist_util.volume_generator(i, device="cpu", draw=d)), s)
    for bad in (-1, dist_util.MAX_DRAW + 1):
        with pytest.raises(ValueError):
            dist_util.volume_generator(0, device="cpu", draw=bad)


def test_draw_seeds_do_not_collide():
    """The seeds of (index, draw), index < 1000003, draw < 64, are pairwise distinct, in 64 bits and in the low 32
    bits the host generator keeps: each draw's block of indices is a run of its own."""
    n = 1000003
    lo = []
    for d in range(_hip.MAX_DRAWS):
        g0 = 10 * 1000003 + d * dist_util.DRAW_SEED_STRIDE
        g1 = g0 + n - 1
        assert g1 < 1 << 32
        lo.append((g0, g1))
    for (a0, a1), (b0, b1) in zip(lo, lo[1:]):
        assert a1 < b0
    # and the generator really uses that seed
    g = dist_util.volume_generator(5, device="cpu", draw=3)
    ref = torch.Generator(device="cpu")
    ref.manual_seed(10 * 1000003 + 5 + 3 * dist_util.DRAW_SEED_STRIDE)
    assert torch.equal(_stream(g), _stream(ref))


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("k", ["0", "-1", "-8", "65"])
def test_script_refuses_bad_num_draws_before_building_a_model(k, tmp_path, monkeypatch):
    mod = _script()

    def no_model(*a, **kw):
        raise AssertionError("a model was built")

    monkeypatch.setattr(mod, "sr_create_model_and_diffusion", no_model)
    monkeypatch.setattr(mod.dist_util, "setup_dist", no_model)
    with pytest.raises(SystemExit) as e:
        mod.main(["--num_draws", k, "--base_samples", str(tmp_path / "none.npz"), "--save_dir", str(tmp_path)])
    assert e.value.code == 2


def test_script_defaults_to_one_draw():
    args = _script().create_argparser().parse_args([])
    assert args.num_draws == 1
