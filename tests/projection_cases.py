"""
The cases of ddpm3d_project shared by the CPU tier (tests/test_projection_cpu.py: the yardstick alone flags at most
1 % of each case's outputs ambiguous) and the GPU tier (tests/test_gpu_projection.py: every other output lies within
the header's bound).  Small on purpose: odd extents, spacings with and without dyadic ratios, both parities of bins
and samples, one bin, a detector too short for the slice, one and three volumes.
"""

import numpy as np

ANGLES = (0.0, 90.0, 180.0, 270.0, 45.0, 33.3, 359.0)

# name: shape (D, H, W), spacing (s0, s1, s2) mm, volumes B, then projection_plan's keywords; "angles" where they are
# not ANGLES
CASES = {
    "one_voxel": dict(shape=(1, 1, 1), spacing=(3.0, 2.0, 2.0), B=1, plan=dict(bins=1, samples=1)),
    "one_voxel_default": dict(shape=(1, 1, 1), spacing=(3.0, 2.0, 2.0), B=1, plan=dict()),
    "3x7x13_iso_default": dict(shape=(3, 7, 13), spacing=(3.0, 2.0, 2.0), B=1, plan=dict()),
    "3x7x13_25_even_odd": dict(shape=(3, 7, 13), spacing=(3.0, 2.5, 2.0), B=3, plan=dict(bins=18, samples=19)),
    "3x7x13_327_fine": dict(shape=(3, 7, 13), spacing=(3.0, 2.0, 3.27), B=1,
                            plan=dict(pitch=1.0, step=0.5, bins=45, samples=88)),
    "3x7x13_327_clipped": dict(shape=(3, 7, 13), spacing=(3.0, 2.0, 3.27), B=1, plan=dict(bins=5, samples=7)),
    "5x9x6_iso_default": dict(shape=(5, 9, 6), spacing=(3.0, 2.0, 2.0), B=3, plan=dict()),
    "5x9x6_327_odd_even": dict(shape=(5, 9, 6), spacing=(3.0, 2.0, 3.27), B=1, plan=dict(bins=15, samples=16)),
    "5x9x6_25_one_bin": dict(shape=(5, 9, 6), spacing=(3.0, 2.5, 2.0), B=1, plan=dict(bins=1, samples=14)),
    "5x9x6_25_many_bins": dict(shape=(5, 9, 6), spacing=(3.0, 2.5, 2.0), B=1, plan=dict(bins=70, samples=12)),
    # more angles than one workgroup walks, and the most the table holds
    "3x7x13_19_angles": dict(shape=(3, 7, 13), spacing=(3.0, 2.0, 2.0), B=1, plan=dict(),
                             angles=tuple(7.5 + 19.0 * k for k in range(19))),
    "1x4x5_64_angles": dict(shape=(1, 4, 5), spacing=(3.0, 2.0, 2.5), B=2, plan=dict(bins=66, samples=5),
                            angles=tuple(360.0 * k / 64 for k in range(64))),
}


def angles_of(case):
    return case.get("angles", ANGLES)

# pitch = step = the (isotropic) in-plane spacing, bins = W and samples = H (mod 2) for the angles along H (0, 180),
# bins = H and samples = W (mod 2) for those along W (90, 270): every sample sits on a voxel, the tables are exact,
# and the MIP is the maximum along the axis.  name: shape, spacing, angles, bins, samples
EXACT_CASES = {
    "3x7x13_all": dict(shape=(3, 7, 13), spacing=(3.0, 2.0, 2.0), angles=(0.0, 90.0, 180.0, 270.0), bins=15,
                       samples=15),
    "5x9x6_along_h": dict(shape=(5, 9, 6), spacing=(3.0, 2.0, 2.0), angles=(0.0, 180.0), bins=8, samples=11),
    "5x9x6_along_w": dict(shape=(5, 9, 6), spacing=(3.0, 2.0, 2.0), angles=(90.0, 270.0), bins=11, samples=8),
    "5x9x6_short": dict(shape=(5, 9, 6), spacing=(3.0, 0.5, 0.5), angles=(0.0, 180.0), bins=4, samples=9),
}


def volumes(name, B, shape):
    """B reproducible volumes of a case: positive, PET-like spread, no two voxels equal"""
    seed = sum(ord(c) for c in name)
    rng = np.random.default_rng(seed)
    return rng.gamma(2.0, 1.5, size=(B,) + tuple(shape)).astype(np.float32)


def amax_image(vol, along, bins):
    """what an exact case's MIP must be: vol (D, H, W) -> (D, bins), the maximum along axis `along` (1: H, the rays
    of 0 degrees; 2: W, those of 90), centred on the detector, 0 beside the slice"""
    return axis_image(vol.max(axis=along), bins)


def axis_image(reduced, bins):
    """(D, n) values per column of voxels -> (D, bins): centred on a detector of the same parity, 0 beside the slice"""
    n = reduced.shape[1]
    out = np.zeros((reduced.shape[0], bins), dtype=reduced.dtype)
    first = (bins - n) // 2                                 # same parity: the centres coincide
    lo, hi = max(first, 0), min(first + n, bins)
    out[:, lo:hi] = reduced[:, lo - first:hi - first]
    return out
