"""
The layout kernels around the network -- ddpm3d_ncdhw_to_ndhwc_pad (how an input that is not the two-plane SuperRes pair
enters the net), ddpm3d_ncdhw_to_ndhwc / ddpm3d_ndhwc_to_ncdhw (the 32 x 32 LDS-tiled transpose) and
ddpm3d_subsample_hw2 -- bit for bit against torch indexing: one element and one tile, sizes one below, at and one above
the 32-wide tile and the 256-thread block, more than one block, more than one sample.  Inputs carry NaN, +-Inf and
-0.0 among ordinary values, outputs start NaN-filled with NaN-filled floats behind them: every element must be
written, with the input's bits, and nothing behind the output.

Left out: the second pass of ddpm3d_subsample_hw2's grid-stride loop, which takes more than 65 536 x 256 output quads
(a 268 MB output from a gigabyte of input).
"""

import numpy as np
import pytest
import torch

from guided_diffusion import _hip as H

pytestmark = pytest.mark.gpu

TAIL = 64
EINVAL = -1


def values(shape, seed):
    """standard normal fp32 with NaN, +Inf, -Inf and -0.0 at seeded places"""
    g = np.random.default_rng(seed)
    x = g.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 8:
        at = g.choice(flat.size, 4, replace=False)
        flat[at] = [np.nan, np.inf, -np.inf, -0.0]
    return torch.from_numpy(x).cuda()


def nan_buf(n):
    return torch.full((n + TAIL,), float("nan"), device="cuda")


def same_bits(got, expect):
    return torch.equal(got.contiguous().view(torch.int32), expect.contiguous().view(torch.int32))


def written(buf, expect):
    """buf holds expect's bits and NaN behind them"""
    n = expect.numel()
    return same_bits(buf[:n], expect.reshape(-1)) and bool(torch.isnan(buf[n:]).all())


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C,Cpad", [(1, 16), (2, 16), (3, 4), (16, 16), (5, 32)])
def test_ncdhw_to_ndhwc_pad(C, Cpad, N):
    lib = H.load()
    for voxels in (1, 255, 256, 257, 1000):
        x = values((N, C, voxels), [C, Cpad, N, voxels])
        expect = torch.zeros(N, voxels, Cpad, device="cuda")           # pad lanes: +0.0
        expect[:, :, :C] = x.permute(0, 2, 1)
        out = nan_buf(N * voxels * Cpad)
        H.check(lib.ddpm3d_ncdhw_to_ndhwc_pad(H.ptr(x), N, C, voxels, Cpad, H.ptr(out), H.stream()))
        assert written(out, expect), (N, C, Cpad, voxels)


def test_ncdhw_to_ndhwc_pad_refuses_a_pad_below_the_channels():
    lib = H.load()
    x = values((2, 5, 300), 1)
    out = nan_buf(2 * 300 * 5)
    for Cpad in (4, 1, 0, -16):
        assert lib.ddpm3d_ncdhw_to_ndhwc_pad(H.ptr(x), 2, 5, 300, Cpad, H.ptr(out), H.stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("C", [1, 31, 32, 33, 64, 100])
def test_transposes_and_their_round_trip(C):
    lib, N = H.load(), 2
    for voxels in (1, 31, 32, 33, 1025):
        x = values((N, C, voxels), [C, voxels])
        y = nan_buf(N * C * voxels)
        H.check(lib.ddpm3d_ncdhw_to_ndhwc(H.ptr(x), N, C, voxels, H.ptr(y), H.stream()))
        assert written(y, x.permute(0, 2, 1)), (C, voxels)
        z = nan_buf(N * C * voxels)
        H.check(lib.ddpm3d_ndhwc_to_ncdhw(H.ptr(y), N, C, voxels, H.ptr(z), H.stream()))
        assert written(z, x), (C, voxels)
        # the channels-last tensor on its own: [N, voxels, C] -> [N, C, voxels]
        w = values((N, voxels, C), [voxels, C, 1])
        v = nan_buf(N * C * voxels)
        H.check(lib.ddpm3d_ndhwc_to_ncdhw(H.ptr(w), N, C, voxels, H.ptr(v), H.stream()))
        assert written(v, w.permute(0, 2, 1)), (C, voxels)


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("D,Hh,W,C", [(1, 2, 2, 4), (3, 6, 10, 4), (2, 4, 2, 36), (5, 2, 14, 8)])
def test_subsample_hw2(D, Hh, W, C, N):
    """out[n, z, y, x, :] = in[n, z, 2y, 2x, :]; the loop's second grid pass is left out (module docstring)."""
    lib = H.load()
    x = values((N, D, Hh, W, C), [N, D, Hh, W, C])
    out = nan_buf(N * D * (Hh // 2) * (W // 2) * C)
    H.check(lib.ddpm3d_subsample_hw2(H.ptr(x), N, D, Hh, W, C, H.ptr(out), H.stream()))
    assert written(out, x[:, :, ::2, ::2, :]), (N, D, Hh, W, C)
