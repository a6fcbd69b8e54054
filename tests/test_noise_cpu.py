"""
Keyed sampler noise without a GPU: the reference generator against the published known answers, the
statistics of the reference stream, the C ABI's host-side refusals (no kernel is launched), and the host classes'
and the script's argument checks.
"""

import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import noise_ref as NR
from conftest import PKG, ROOT
from guided_diffusion import _hip, dist_util, joint
from guided_diffusion.gaussian_diffusion import GaussianDiffusion, NoiseKey

NEW = ["ddpm3d_noise_fill", "ddpm3d_noise_bits", "ddpm3d_p_sample_step_keyed", "ddpm3d_ddim_step_keyed",
       "ddpm3d_dpm_solver_step_keyed", "ddpm3d_q_sample_keyed"]


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("key, counter, out", [
    ((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 2, (0xffffffff,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(key, counter, out):
    assert _hex(np.ravel(NR.philox(*counter, *key))) == out
    # the same through the (seed, stream, draw, q) packing of the noise function
    seed, stream = key[0] | (key[1] << 32), counter[2] | (counter[3] << 32)
    assert _hex(NR.words(seed, stream, counter[1], np.array([counter[0]]))[0]) == out


def test_abi_stays_13_and_the_new_names_are_exported():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    assert re.search(r"#define\s+DDPM3D_ABI_VERSION\s+13\b", hdr)
    assert _hip.ABI_VERSION == 13
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ddpm3d_abi_version.restype = ctypes.c_int
    assert lib.ddpm3d_abi_version() == 13
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    # struct ddpm3d_noise_key: 8 + 8 + 8 + 8 + 12 + 12 bytes, fields in the header's order
    assert ctypes.sizeof(_hip.NoiseKeyDesc) == 56
    assert [f[0] for f in _hip.NoiseKeyDesc._fields_] == ["seed", "stream", "draw", "origin", "patch", "canvas"]


def _lib():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW + ["ddpm3d_last_error"]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _hip.EXPORTS[name]
    return lib


class _Host:
    """Pointers to host memory: every call below must return before it would launch anything."""

    def __init__(self):
        self.buf = (ctypes.c_float * 4096)()
        self.p = ctypes.addressof(self.buf)

    def key(self, stream=True, draw=0, origin=False, patch=(0, 0, 0), canvas=(0, 0, 0)):
        k = _hip.NoiseKeyDesc()
        k.seed, k.draw = 10, draw
        k.stream = self.p if stream else None
        k.origin = self.p if origin else None
        for a in range(3):
            k.patch[a], k.canvas[a] = patch[a], canvas[a]
        return k


BAD_KEYS = {
    "null stream": dict(stream=False),
    "negative draw": dict(draw=-1),
    "draw 2^32": dict(draw=2 ** 32),
    "patch extent 0": dict(origin=True, patch=(4, 0, 16), canvas=(8, 8, 8)),
    "canvas extent 0": dict(origin=True, patch=(4, 4, 4), canvas=(8, 0, 8)),
    "negative canvas": dict(origin=True, patch=(4, 4, 4), canvas=(8, -8, 8)),
    "patch product is not voxels": dict(origin=True, patch=(4, 4, 5), canvas=(8, 8, 8)),
    "index range reaches 2^34": dict(origin=True, patch=(4, 4, 4), canvas=(4096, 2048, 2049)),
}


def _entries(lib, h, key, N=2, voxels=64):
    """Every keyed entry on (key, N, voxels), the other arguments valid."""
    kp = None if key is None else ctypes.byref(key)
    p = h.p
    return {
        "noise_fill": lambda: lib.ddpm3d_noise_fill(kp, N, voxels, p, None),
        "noise_bits": lambda: lib.ddpm3d_noise_bits(kp, N, voxels, p, None),
        "p_sample_step_keyed": lambda: lib.ddpm3d_p_sample_step_keyed(p, p, kp, p, p, N, voxels, 0, p, p, None),
        "ddim_step_keyed": lambda: lib.ddpm3d_ddim_step_keyed(p, p, kp, p, p, N, voxels, 0, 0.5, p, p, None),
        "dpm_solver_step_keyed": lambda: lib.ddpm3d_dpm_solver_step_keyed(p, p, None, None, kp, p, p, p, N, voxels, 10,
                                                                           0, 1, p, p, None),
        "q_sample_keyed": lambda: lib.ddpm3d_q_sample_keyed(p, kp, p, p, N, voxels, 10, p, None),
    }


@pytest.mark.parametrize("case", sorted(BAD_KEYS))
def test_every_entry_refuses_a_bad_key_without_a_gpu(case):
    lib, h = _lib(), _Host()
    key = h.key(**BAD_KEYS[case])
    for name, call in _entries(lib, h, key).items():
        if name == "noise_bits" and BAD_KEYS[case].get("origin"):
            continue                                   # reads seed, stream and draw only
        assert call() == _hip.E_INVAL, (case, name)
        assert lib.ddpm3d_last_error().decode().startswith(name + ":"), (case, name, lib.ddpm3d_last_error())


def test_entries_refuse_null_key_and_bad_counts_without_a_gpu():
    lib, h = _lib(), _Host()
    for name, call in _entries(lib, h, None).items():
        if name != "dpm_solver_step_keyed":            # there a NULL key is the ODE form
            assert call() == _hip.E_INVAL, name
    good = h.key()
    for N, voxels in ((0, 64), (-1, 64), (2, 0), (2, -5), (65536, 64)):
        for name, call in _entries(lib, h, good, N, voxels).items():
            assert call() == _hip.E_INVAL, (name, N, voxels)
    # a canvas of exactly 2^34 voxels is the largest a stream can index: the refusal below is then the NULL output,
    # not the key
    edge = h.key(origin=True, patch=(4, 4, 4), canvas=(4096, 2048, 2048))
    assert lib.ddpm3d_noise_fill(ctypes.byref(edge), 2, 64, None, None) == _hip.E_INVAL
    assert lib.ddpm3d_last_error().decode() == "noise_fill: NULL out"
    assert lib.ddpm3d_noise_bits(ctypes.byref(good), 2, 64, None, None) == _hip.E_INVAL


def test_noise_stream_values():
    assert dist_util.noise_stream(0) == 0
    assert dist_util.noise_stream(7, 0) == 7
    assert dist_util.noise_stream(7, 3) == 7 + (3 << 32)
    # none of volume_generator's limits: patch indices of 2^24 and above, draws above 255
    assert dist_util.noise_stream(3 * 2 ** 24 + 7, 256) == 3 * 2 ** 24 + 7 + (256 << 32)
    assert dist_util.noise_stream(2 ** 32 - 1, 2 ** 32 - 1) == 2 ** 64 - 1
    seen = {dist_util.noise_stream(i, d) for i in (0, 1, 2 ** 24, 2 ** 32 - 1) for d in (0, 1, 255, 256, 2 ** 31)}
    assert len(seen) == 20
    for bad in ((-1, 0), (2 ** 32, 0), (0, -1), (0, 2 ** 32)):
        with pytest.raises(ValueError):
            dist_util.noise_stream(*bad)
    assert dist_util.MAX_DRAW == 255 and dist_util.DRAW_SEED_STRIDE == 1 << 24      # volume_generator stays


def test_noise_key_argument_checks():
    for seed in (-1, 2 ** 64, 1.5, True, "10"):
        with pytest.raises(ValueError):
            NoiseKey(seed, [0])
    for streams in ([], [0.5], [True], [2 ** 64], [-2 ** 63 - 1], ["a"]):
        with pytest.raises(ValueError):
            NoiseKey(10, streams)
    with pytest.raises(ValueError):
        NoiseKey(10, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        NoiseKey(10, torch.zeros(2, dtype=torch.int64))            # a host tensor
    geo = dict(origin=[(0, 0, 0)], patch=(4, 4, 4), canvas=(8, 8, 8))
    for drop in geo:                                               # the three come together
        with pytest.raises(ValueError):
            NoiseKey(10, [0], **{k: v for k, v in geo.items() if k != drop})
    for over in (dict(patch=(4, 4)), dict(patch=(4, 0, 4)), dict(canvas=(8, 8, -8)), dict(origin=[(0, 0)]),
                 dict(origin=[(0, 0, 0), (1, 1, 1)]), dict(canvas=(4096, 2048, 2049)),
                 dict(origin=[(2 ** 31, 0, 0)])):
        with pytest.raises(ValueError):
            NoiseKey(10, [0], **dict(geo, **over))


def test_every_loop_takes_noise_key():
    names = ["p_sample_loop", "ddim_sample_loop", "dpm_solver_sample_loop"]
    fns = [getattr(GaussianDiffusion, n + s) for n in names for s in ("", "_progressive")]
    fns += [GaussianDiffusion.calc_bpd_loop, GaussianDiffusion.p_sample, GaussianDiffusion.ddim_sample,
            GaussianDiffusion.q_sample, joint.sample_loop_progressive]
    for fn in fns:
        p = inspect.signature(fn).parameters
        assert "noise_key" in p and p["noise_key"].default is None, fn


def test_noise_key_with_step_noise_is_refused_before_anything_runs():
    d = GaussianDiffusion.__new__(GaussianDiffusion)
    key = NoiseKey.__new__(NoiseKey)
    with pytest.raises(ValueError, match="noise_key"):
        GaussianDiffusion._check_key(key, [None])
    with pytest.raises(ValueError, match="NoiseKey"):
        GaussianDiffusion._check_key(object(), None)
    GaussianDiffusion._check_key(None, [None])
    GaussianDiffusion._check_key(key, None)
    for loop in (d.p_sample_loop, d.ddim_sample_loop, d.dpm_solver_sample_loop):
        with pytest.raises(ValueError, match="noise_key"):
            loop(None, (1, 1, 4, 4, 4), step_noise=[None], noise_key=key)


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_flags_and_refusals(capsys):
    mod = _script()
    p = mod.create_argparser()
    a = p.parse_args([])
    assert a.device_noise is False and a.noise_seed == 10
    a = p.parse_args(["--device_noise", "True", "--noise_seed", "11"])
    assert a.device_noise is True and a.noise_seed == 11
    # without --device_noise the old path's seed is the literal it was: another one is refused before the model is built
    for argv in (["--noise_seed", "11"], ["--device_noise", "False", "--noise_seed", "0"],
                 ["--device_noise", "True", "--noise_seed", "-1"],
                 ["--device_noise", "True", "--noise_seed", str(2 ** 64)]):
        with pytest.raises(SystemExit) as e:
            mod.main(argv)
        assert e.value.code == 2
        assert "--noise_seed" in capsys.readouterr().err


# ------------------------------------------------------------- statistics of the reference stream
N_STAT = 1 << 20


@pytest.fixture(scope="module")
def streams():
    return {name: NR.normals(seed, stream, draw, N_STAT)
            for name, (seed, stream, draw) in {"base": (10, 0, 0), "draw 1": (10, 0, 1), "stream 1": (10, 1, 0),
                                               "seed 11": (11, 0, 0)}.items()}


def test_reference_stream_statistics(streams):
    """Every statistic within 5 of its own standard deviation (1/sqrt(n) for the mean and the products of independent
    unit normals, sqrt(2/n) for the variance, sqrt(96/n) for the fourth moment): a condition a broken mapping -- a
    repeated word, a shared counter, a lane used twice -- misses by hundreds."""
    z, n = streams["base"], float(N_STAT)
    stats = {
        "mean": z.mean() * np.sqrt(n),
        "variance": ((z * z).mean() - 1.0) / np.sqrt(2.0 / n),
        "fourth moment": ((z ** 4).mean() - 3.0) / np.sqrt(96.0 / n),
        "product with draw 1": (z * streams["draw 1"]).mean() * np.sqrt(n),
        "product with stream 1": (z * streams["stream 1"]).mean() * np.sqrt(n),
        "product with seed 11": (z * streams["seed 11"]).mean() * np.sqrt(n),
    }
    for lag in (1, 2, 4):
        stats["lag %d" % lag] = (z[:-lag] * z[lag:]).mean() * np.sqrt(n)
    for name, v in stats.items():
        print("%-22s %+.2f" % (name, v))
    for name, v in stats.items():
        assert abs(v) <= 5.0, (name, v)
    assert np.isfinite(z).all()
    assert np.abs(z).max() <= np.sqrt(66.0 * np.log(2.0))
    print("max |z| %.3f" % np.abs(z).max())


def test_reference_normals_extremes_and_index_rule():
    # u1 never 0: the smallest word gives 2^-33, the largest rounds to 1 (r = 0)
    u1, u2 = NR.uniforms(np.array([0, 2 ** 32 - 1], dtype=np.uint64), np.array([0, 2 ** 32 - 1], dtype=np.uint64))
    assert u1[0] == 2.0 ** -33 and u1[1] == 1.0 and u2[0] == 0.0 and u2[1] == 1.0 - 2.0 ** -32
    assert np.sqrt(-2.0 * np.log(u1[0])) == pytest.approx(np.sqrt(66.0 * np.log(2.0)))
    # lanes: indices 4q .. 4q + 3 share counter q; any subset of indices gives the same values
    full = NR.normals(10, 5, 2, 64)
    idx = np.array([63, 0, 17, 18, 2], dtype=np.uint64)
    assert np.array_equal(NR.normals_at(10, 5, 2, idx), full[idx.astype(int)])
    # the geometry index of a patch voxel
    ci = NR.canvas_index((1, 3, 5), (4, 4, 4), (5, 7, 9))
    assert ci.shape == (4, 4, 4) and ci[0, 0, 0] == (1 * 7 + 3) * 9 + 5 and ci[3, 3, 3] == (4 * 7 + 6) * 9 + 8
