"""
Yardstick of the patch gather and blend entries for B canvases at once: the numpy restatements
patches.joint_gather / patches.joint_blend, draw by draw, in the entries' (patch, draw)-major row order.
"""

import numpy as np

from guided_diffusion import patches


def np_gather(canvases, geom):
    """(B, Dc, H, W) -> (P * B, 1, res, res, res): patch-major, draw-minor"""
    per_draw = np.stack([patches.joint_gather(c, geom) for c in canvases], axis=1)       # (P, B, 1, r, r, r)
    return per_draw.reshape((-1,) + per_draw.shape[2:])


def np_blend(rows, geom, B):
    """(P * B, 1, res, res, res) -> (B, Dc, H, W)"""
    r = geom.res
    per = rows.reshape(geom.n_patches, B, 1, r, r, r)
    return np.stack([patches.joint_blend(per[:, b], geom) for b in range(B)])
