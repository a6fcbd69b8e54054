"""
GPU tier of the halo-tile frame shared by ddpm3d_sphere_mean and ddpm3d_nlm (csrc/halo_tile.h): every
tile and LDS-budget class of either kernel (tests/halo_tile_cases.py) within the entry's own bound of its fp64
yardstick, centred and on an offset of 1000; the same outputs plane by plane against the bits of the commit before
the frame was shared (tests/golden/halo_tile_bits.json); one call per kernel that walks more than 65535 tiles along D;
and bit-repeatability of a whole-CU launch, followed by other TD instantiations in the same process.
"""

import json
import os

import numpy as np
import pytest
import torch

import baseline_ref as B
import halo_tile_cases as C
from conftest import GOLDEN
from guided_diffusion import metrics
from test_gpu_baseline import within_bound as nlm_within
from test_gpu_peak import within_bound as peak_within

pytestmark = pytest.mark.gpu

PEAK_IDS = [C.peak_key(c[0], c[1]) for c in C.PEAK_CLASSES]
NLM_IDS = [C.nlm_key(c[0], c[1]) for c in C.NLM_CLASSES]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared references are read-only


def run_peak(keep, radii, offset, shape=C.SHAPE):
    x, mask, half_w, ref = C.peak_case(keep, radii, offset, shape)
    fp = metrics.SphereFootprint(None, None, None, radii, half_w)
    return metrics.sphere_mean(dev(x), fp, keep=None if mask is None else dev(mask)), ref


def run_nlm(search, patch, offset):
    x, h, m, bound, _, _ = B.nlm_case(C.SHAPE, search, patch, offset)
    return metrics.nlm(dev(x), h, search=search, patch=patch), m, bound


@pytest.fixture(scope="module")
def parent_bits():
    """The SHA-256 of every D plane of the 25 centred cases, recorded on an MI355X from the commit before the two
    kernels shared their frame (tests/golden/make_halo_tile_bits.py; the file names the commit and the compiler).
    Non-local means calls expf, so these bits are a property of the toolchain too: after a compiler change they are
    recorded again from the commit before that change."""
    with open(os.path.join(GOLDEN, "halo_tile_bits.json")) as f:
        return json.load(f)["cases"]


def same_planes(got, want, what):
    have = C.plane_digests(got.cpu().numpy())
    assert len(have) == len(want) == C.SHAPE[0]
    first = next((z for z in range(len(have)) if have[z] != want[z]), None)
    assert first is None, "%s: D plane %d is the first that differs from the recorded bits" % (what, first)


# ------------------------------------------------------------------------------------------ every class, the bound
@pytest.mark.parametrize("offset", [0.0, 1000.0], ids=["centred", "offset1000"])
@pytest.mark.parametrize("keep,radii,tile,budget", C.PEAK_CLASSES, ids=PEAK_IDS)
def test_sphere_mean_class_within_the_bound(keep, radii, tile, budget, offset):
    got, ref = run_peak(keep, radii, offset)
    if keep:
        assert (ref[1] == 0).any()                            # the block of zeros leaves voxels that count nothing
    peak_within(got, ref, "sphere mean %s radii %s (%d x %d, %s) offset %g" % ("keep" if keep else "all", radii,
                                                                              *tile, budget, offset))


@pytest.mark.parametrize("offset", [0.0, 1000.0], ids=["centred", "offset1000"])
@pytest.mark.parametrize("search,patch,tile,budget,raised", C.NLM_CLASSES, ids=NLM_IDS)
def test_nlm_class_within_the_bound(search, patch, tile, budget, raised, offset):
    got, m, bound = run_nlm(search, patch, offset)
    nlm_within(got, m, bound, "nlm search %s patch %s (%d x %d, %s%s) offset %g"
               % (search, patch, *tile, budget, ", limit raised" if raised else "", offset))


# ------------------------------------------------------------------------------------------ the parent's bits
@pytest.mark.parametrize("keep,radii,tile,budget", C.PEAK_CLASSES, ids=PEAK_IDS)
def test_sphere_mean_class_has_the_recorded_bits(keep, radii, tile, budget, parent_bits):
    key = C.peak_key(keep, radii)
    same_planes(run_peak(keep, radii, 0.0)[0], parent_bits[key], key)


@pytest.mark.parametrize("search,patch,tile,budget,raised", C.NLM_CLASSES, ids=NLM_IDS)
def test_nlm_class_has_the_recorded_bits(search, patch, tile, budget, raised, parent_bits):
    key = C.nlm_key(search, patch)
    same_planes(run_nlm(search, patch, 0.0)[0], parent_bits[key], key)


# ------------------------------------------------------------------------------------------ the D stride loop
def test_sphere_mean_walks_more_tiles_along_d_than_a_grid_holds():
    shape, radii = C.PEAK_LONG
    got, ref = run_peak(False, radii, 0.0, shape)
    peak_within(got, ref, "sphere mean %s radii %s" % (shape, radii))


def test_nlm_walks_more_tiles_along_d_than_a_grid_holds():
    shape, search, patch = C.NLM_LONG
    x, h, m, bound = C.nlm_long_case(shape, search, patch)
    nlm_within(metrics.nlm(dev(x), h, search=search, patch=patch), m, bound, "nlm %s search %s patch %s"
               % (shape, search, patch))


# ------------------------------------------------------------------------------------------ repeatability
def test_whole_cu_launches_repeat_and_do_not_serve_another_td(parent_bits):
    """a whole-CU case twice, bit for bit; then cases of other TD in the same process, one of them a whole-CU case of
    its own: the once-per-device raise of one instantiation is not taken for another's"""
    first = run_peak(True, (4, 5, 1), 0.0)[0]                # 8 x 8, whole CU
    assert torch.equal(first.view(torch.int32), run_peak(True, (4, 5, 1), 0.0)[0].view(torch.int32))
    for keep, radii in ((True, (3, 6, 1)), (True, (8, 8, 2)), (True, (6, 8, 2))):     # 1 x 4 small; 4 x 4, 4 x 8 whole
        key = C.peak_key(keep, radii)
        same_planes(run_peak(keep, radii, 0.0)[0], parent_bits[key], key)
    first = run_nlm((5, 5, 5), (2, 2, 1), 0.0)[0]             # 8 x 8, whole CU
    assert torch.equal(first.view(torch.int32), run_nlm((5, 5, 5), (2, 2, 1), 0.0)[0].view(torch.int32))
    for search, patch in (((4, 5, 3), (0, 2, 1)), ((4, 5, 1), (1, 2, 0)), ((5, 5, 3), (2, 2, 1))):
        key = C.nlm_key(search, patch)                        # 4 x 4 plain; 4 x 4 and 1 x 4 with the limit raised
        same_planes(run_nlm(search, patch, 0.0)[0], parent_bits[key], key)
