"""
The cases of tests/test_gpu_halo_tile.py and of tests/golden/make_halo_tile_bits.py: one case per tile and LDS-budget
class of the two halo-tile kernels (csrc/halo_tile.h), on a volume of (10, 9, 66): two tiles with a
ragged second one along every axis for the 8 x 8 x 64 tile, and thinner than the larger halos along D and H.  Inputs
and references come from the yardsticks' seeded numpy generators (peak_ref, baseline_ref), so they are the same on any
machine; host arithmetic only.

The tile, budget and limit-raised columns of PEAK_CLASSES and NLM_CLASSES only describe a case and label its test:
nothing here checks them, and the pick functions are local to peak.hip and nlm.hip.  They were confirmed once by
enumerating the radii against those functions on the host; a later change to a tile list or a budget is not caught
here and wants the two tables worked out again.
"""

import functools
import hashlib
import itertools
import math

import numpy as np

import baseline_ref as B
import peak_ref as P

SHAPE = (10, 9, 66)

# keep, (r0, r1, rw), tile, budget: the smallest radii with a W halo of at least 1 that take each class (small = 40 KB,
# four workgroups per CU; whole = the LDS limit is raised); last the case without tail words, rw = 0
PEAK_CLASSES = [
    (False, (0, 0, 1), (8, 8), "small"),
    (False, (1, 4, 1), (4, 8), "small"),
    (False, (3, 4, 1), (4, 4), "small"),
    (False, (3, 6, 1), (2, 4), "small"),
    (False, (4, 6, 1), (1, 4), "small"),
    (False, (5, 5, 1), (8, 8), "whole"),
    (False, (8, 8, 4), (4, 8), "whole"),
    (True, (0, 0, 1), (8, 8), "small"),
    (True, (0, 4, 1), (4, 8), "small"),
    (True, (2, 4, 1), (4, 4), "small"),
    (True, (2, 6, 1), (2, 4), "small"),
    (True, (3, 6, 1), (1, 4), "small"),
    (True, (4, 5, 1), (8, 8), "whole"),
    (True, (6, 8, 2), (4, 8), "whole"),
    (True, (8, 8, 2), (4, 4), "whole"),
    (True, (1, 1, 0), (8, 8), "small"),
]
# search, patch (halo R_a = s_a + p_a, patch radii that differ per axis where they can), tile, budget, limit raised
NLM_CLASSES = [
    ((0, 0, 1), (0, 0, 0), (8, 8), "80 KB", False),
    ((2, 3, 1), (1, 2, 0), (8, 8), "80 KB", True),
    ((4, 3, 1), (2, 1, 0), (8, 4), "80 KB", False),
    ((3, 4, 1), (1, 2, 0), (8, 4), "80 KB", True),
    ((4, 5, 3), (0, 2, 1), (4, 4), "80 KB", False),
    ((4, 5, 1), (1, 2, 0), (4, 4), "80 KB", True),
    ((5, 5, 1), (2, 2, 0), (2, 4), "80 KB", True),
    ((5, 5, 3), (2, 2, 1), (1, 4), "80 KB", True),
    ((5, 5, 5), (2, 2, 1), (8, 8), "whole", True),
]
# the D stride loop: more than 65535 tiles of 1 x 4 x 64 along D
PEAK_LONG = ((65540, 1, 3), (4, 6, 1))
NLM_LONG = ((65540, 1, 1), (5, 5, 3), (2, 2, 1))


def peak_key(keep, radii):
    return "sphere_mean-%s-%d.%d.%d" % ("keep" if keep else "all", *radii)


def nlm_key(search, patch):
    return "nlm-s%d.%d.%d-p%d.%d.%d" % (*search, *patch)


def ellipsoid(radii):
    """a symmetric half_w table ((2 r0 + 1) x (2 r1 + 1)) with every row of the box's axes present and the largest
    half-width, rw, on the centre row: the ellipsoid with semi-axes r_a + 1/2"""
    r0, r1, rw = radii
    rows = []
    for dz in range(-r0, r0 + 1):
        rows.append([])
        for dy in range(-r1, r1 + 1):
            q = (dz / (r0 + 0.5)) ** 2 + (dy / (r1 + 0.5)) ** 2
            rows[-1].append(min(rw, int((rw + 0.5) * math.sqrt(1.0 - q))) if q <= 1.0 else -1)
    assert rows[r0][r1] == rw and rows[0][r1] >= 0 and rows[r0][0] >= 0
    return tuple(tuple(row) for row in rows)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def peak_case(keep, radii, offset, shape=SHAPE):
    """one shared, read-only reference: (x fp32, keep uint8 or None, half_w, (mean, n, bound))"""
    half_w = ellipsoid(radii)
    x = P.data(shape, 41, offset)
    mask = P.keep_mask(shape, radii, 43) if keep else None
    ref = P.sphere_mean(x, P.expand(radii, half_w), mask)
    _frozen(x, mask, *ref)
    return x, mask, half_w, ref


@functools.lru_cache(maxsize=None)
def nlm_long_case(shape, search, patch):
    """baseline_ref.nlm_case for a (D, 1, 1) volume: a candidate off the D axis lies outside the volume and counts
    nothing (its weight is dropped and it is in neither n_s nor the median), so only the 2 s0 + 1 candidates along D
    are formed -> (x fp32, h, m, bound)"""
    assert shape[1] == shape[2] == 1
    x = B.spiked(shape, 47)
    _, shifted = B._padded(x, search, patch)
    dist = [(s, B.patch_distance(shifted, s, patch)) for s in itertools.product(range(-search[0], search[0] + 1), [0], [0])]
    h = float(np.float32(B.median_distance(x, search, patch, dist)))
    m, bound, _, _ = B.nlm(x, search, patch, h, 0.0, dist)
    _frozen(x, m, bound)
    return x, h, m, bound


def plane_digests(out):
    """the SHA-256 of every D plane of a (D, H, W) fp32 array"""
    out = np.ascontiguousarray(out, dtype=np.float32)
    return [hashlib.sha256(out[z].tobytes()).hexdigest() for z in range(out.shape[0])]
