"""
numpy reference of the keyed sampler noise (include/ddpm3d.h): Philox4x32-10 on uint64 arrays, the
Box-Muller normals in fp64 from the fp32-rounded u1 and the exact u2 the device function defines, and the canvas
index of a patch voxel.  Written from Salmon et al. (SC'11) and the header's text; shares no code with the library.
"""

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: counter words c0..c3 and key words k0, k1 (arrays or scalars below 2^32) -> four uint64 arrays
    holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def words(seed, stream, draw, quads):
    """(quads, 4) uint32: the words of counters q = 0 .. quads - 1, or of the counters in the array `quads`."""
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    q = np.arange(quads, dtype=np.uint64) if np.isscalar(quads) else np.asarray(quads, dtype=np.uint64)
    w = philox(q, int(draw), stream & 0xFFFFFFFF, stream >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=-1).astype(np.uint32)


def uniforms(wa, wb):
    """(u1, u2) in fp64 of word pairs: u1 = the fp32 value fmaf((float)w_a, 2^-32, 2^-33) -- (float)w_a rounds to
    nearest-even, the scaled sum is exact in fp64 and rounds to fp32 once --, u2 = w_b 2^-32 exactly."""
    fa = wa.astype(np.uint32).astype(np.float32).astype(np.float64)
    u1 = (fa * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)
    return u1, wb.astype(np.float64) * 2.0 ** -32


def normals_at(seed, stream, draw, index, with_r=False):
    """fp64 normals of the voxel indices `index` (any shape, below 2^34) of one stream; with_r also returns
    r = sqrt(-2 ln u1), the scale of the device function's error bound."""
    index = np.asarray(index, dtype=np.uint64)
    w = words(seed, stream, draw, index >> np.uint64(2)).astype(np.uint64)
    high = (index & np.uint64(2)) != 0
    u1, u2 = uniforms(np.where(high, w[..., 2], w[..., 0]), np.where(high, w[..., 3], w[..., 1]))
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    z = r * np.where((index & np.uint64(1)) != 0, np.sin(ang), np.cos(ang))
    return (z, r) if with_r else z


def normals(seed, stream, draw, voxels, with_r=False):
    """fp64 normals of indices 0 .. voxels - 1."""
    return normals_at(seed, stream, draw, np.arange(voxels, dtype=np.uint64), with_r)


def canvas_index(origin, patch, canvas):
    """(pd, ph, pw) int64 linear canvas indices of the voxels of the patch at origin (z0, y0, x0)."""
    z0, y0, x0 = (int(v) for v in origin)
    _, Hc, Wc = canvas
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in patch], indexing="ij")
    return ((z0 + z) * Hc + y0 + y) * Wc + x0 + x
