"""
Whole-body volume <-> 96^3 sub-volume patches: the steps either side of the
sampling hot path in the reference's inference script.

Restated from scripts/test.py:185-246 (tiling), :248-262 (3-D Hann window),
:92-146 (weighted overlap-add) and :283-301 (start positions).  scripts/test.py
cannot be imported in the build container (it needs tifffile / mpi4py) and the
reference holds no fixtures for it, so every function here is pinned to
outputs of the reference's OWN code, taken out of the script's syntax tree
and run unchanged (tests/golden/make_golden.py): the three pure helpers
(hann_window_3d, xy_starts, z_starts; script_helpers.npz) and the tiling /
overlap-add loop nests that are inline in load_data_for_worker and main()
(split_volume, stitch_patches; script_tiling.npz), bit for bit
(tests/test_patches_cpu.py).  One intended difference: voxels whose total
weight is 0 are 0 here, uninitialised memory in the reference (np.divide with
`where` and no `out`).

Host-side numpy on purpose: this is file-format glue around the GPU path (a
200x200x130 volume is 5 M voxels), exactly where the reference has it.
"""

import numpy as np


def xy_starts(dim_size, patch_size, num_patches=3):
    """scripts/test.py:283-293: fixed number of patches per axis."""
    if dim_size == 200 and patch_size == 96 and num_patches == 3:
        return [0, 52, 104]
    if num_patches == 1:
        return [0]
    step = (dim_size - patch_size) / (num_patches - 1)
    starts = [int(i * step) for i in range(num_patches)]
    starts[-1] = min(starts[-1], dim_size - patch_size)
    return starts


def z_starts(dim_size, patch_size):
    """scripts/test.py:295-301: one patch, or first + last with overlap."""
    if dim_size <= patch_size:
        return [0]
    return [0, dim_size - patch_size]


def patch_grid(shape_dhw, resolution, num_xy=3):
    """[(x_start, y_start, z_start)] in the reference's nesting order (x, y, z)."""
    D, H, W = shape_dhw
    return [(xs, ys, zs) for xs in xy_starts(H, resolution, num_xy)
            for ys in xy_starts(W, resolution, num_xy) for zs in z_starts(D, resolution)]


def sliding_starts(extent, res, min_overlap):
    """Gap-free patch starts along one axis of any length: [0] when one (zero-padded) patch holds
    the axis, otherwise the fewest evenly spread starts, first 0 and last extent - res, whose neighbours overlap by
    at least min_overlap.  min_overlap is in 2..res - 1: np.hanning is 0 at both ends of a patch, so an overlap of
    0 or 1 can leave planes inside the volume without any weight."""
    extent, res, min_overlap = int(extent), int(res), int(min_overlap)
    if extent < 1 or res < 1:
        raise ValueError("sliding_starts: bad axis (extent %d, patch size %d)" % (extent, res))
    if not 2 <= min_overlap <= res - 1:
        raise ValueError("sliding_starts: the overlap must be in 2..%d (patch size %d), got %d"
                         % (res - 1, res, min_overlap))
    if extent <= res:
        return [0]
    span, stride = extent - res, res - min_overlap
    n = (span + stride - 1) // stride + 1
    return [(i * span) // (n - 1) for i in range(n)]


def sliding_grid(shape_dhw, res, min_overlap):
    """[(x_start, y_start, z_start)] of the sliding tiling, in patch_grid's nesting order (x, y, z)."""
    D, H, W = shape_dhw
    return [(xs, ys, zs) for xs in sliding_starts(H, res, min_overlap)
            for ys in sliding_starts(W, res, min_overlap) for zs in sliding_starts(D, res, min_overlap)]


def grid_gaps(shape_dhw, res, num_xy=3):
    """Coordinates per axis {"D": n, "H": n, "W": n} that no patch of patch_grid covers (all 0: the fixed grid
    tiles the volume).  A voxel is written by the one-shot stitcher only if all three of its coordinates are
    covered."""
    D, H, W = (int(v) for v in shape_dhw)
    gaps = {}
    for axis, extent, starts in (("D", D, z_starts(D, res)), ("H", H, xy_starts(H, res, num_xy)),
                                 ("W", W, xy_starts(W, res, num_xy))):
        cover = np.zeros(extent, dtype=bool)
        for s in starts:
            cover[max(s, 0):max(s + res, 0)] = True
        gaps[axis] = int((~cover).sum())
    return gaps


def split_volume(vol, resolution, num_xy=3):
    """(D,H,W) volume -> (P, 1, Z, H, W) float32 zero-padded patches + the grid.
    (The reference routes through an (H,W,Z) transpose and back; the result is the
    same (Z,H,W)-ordered patch.)"""
    vol = np.asarray(vol)
    if vol.ndim == 4 and vol.shape[0] == 1:
        vol = vol[0]
    if vol.ndim != 3:
        raise ValueError("expected a (D,H,W) volume, got shape %s" % (vol.shape,))
    vol = vol.astype(np.float32)
    D, H, W = vol.shape
    grid = patch_grid((D, H, W), resolution, num_xy)
    out = np.zeros((len(grid), 1, resolution, resolution, resolution), dtype=np.float32)
    for i, (xs, ys, zs) in enumerate(grid):
        p = vol[zs:zs + resolution, xs:xs + resolution, ys:ys + resolution]
        out[i, 0, :p.shape[0], :p.shape[1], :p.shape[2]] = p
    return out, grid


def hann_window_3d(size):
    """scripts/test.py:248-262: separable Hann window normalised to max 1."""
    h = np.hanning(size)
    w = np.outer(np.outer(h, h).ravel(), h).reshape(size, size, size)
    return w / w.max()


def stitch_patches(patches_hwz, grid, shape_dhw, resolution):
    """Weighted overlap-add of denoised patches (each (H,W,Z), the layout the
    reference permutes samples into, scripts/test.py:72) into an (H,W,Z) volume.
    Voxels whose total weight is 0 (the outermost planes: np.hanning is 0 at both
    ends) stay 0, as in the reference (np.divide(..., where=weight > 0))."""
    D, H, W = shape_dhw
    acc = np.zeros((H, W, D), dtype=np.float32)
    wsum = np.zeros_like(acc)
    win = hann_window_3d(resolution)
    for patch, (xs, ys, zs) in zip(patches_hwz, grid):
        patch = np.squeeze(np.asarray(patch))
        if patch.ndim != 3:
            raise ValueError("patch has unexpected dimensions: %s" % (patch.shape,))
        xe, ye, ze = min(xs + resolution, H), min(ys + resolution, W), min(zs + resolution, D)
        hx, wy, dz = xe - xs, ye - ys, ze - zs
        acc[xs:xe, ys:ye, zs:ze] += patch[:hx, :wy, :dz] * win[:hx, :wy, :dz]
        wsum[xs:xe, ys:ye, zs:ze] += win[:hx, :wy, :dz]
    return np.divide(acc, wsum, out=acc.copy(), where=wsum > 0), wsum


def blend_cover(grid, shape_dhw, resolution):
    """(H,W,Z) bool: the voxels to which stitch_patches gives a weight above 0 (some patch covers them away from its
    own outermost planes, where the Hann window is 0), known from the grid alone, before any patch is sampled."""
    D, H, W = shape_dhw
    cover = np.zeros((H, W, D), dtype=bool)
    live = hann_window_3d(resolution) > 0
    for xs, ys, zs in grid:
        xe, ye, ze = min(xs + resolution, H), min(ys + resolution, W), min(zs + resolution, D)
        cover[xs:xe, ys:ye, zs:ze] |= live[:xe - xs, :ye - ys, :ze - zs]
    return cover


def blend_shares(starts, extent, res):
    """(len(starts), res) float64: patch i's share of stitch_patches' one-shot Hann blend along one axis, per
    coordinate of the patch: hanning(res)[c - s_i] / sum_j hanning(res)[c - s_j] at c = s_i + column, 0 where that
    sum is 0 (the outermost planes of the volume) and 0 for c >= extent (the zero-padded part of a patch).  The window
    and the grids are separable, so patch p's share of a voxel is the product of three such rows; unlike _axis_table
    no plane gets an equal share: the shares sum to 1 over the patches on the voxels blend_cover marks, to 0 on the
    others."""
    extent, res = int(extent), int(res)
    h = np.hanning(res)
    hann = np.zeros((len(starts), max(extent, 0)), dtype=np.float64)
    for i, s in enumerate(starts):
        n = min(res, extent - s)
        if s < 0 or n < 1:
            raise ValueError("blend_shares: patch start %d outside 0..%d" % (s, extent - 1))
        hann[i, s:s + n] = h[:n]
    total = hann.sum(axis=0)
    live = total > 0
    share = np.where(live, hann / np.where(live, total, 1.0), 0.0)
    out = np.zeros((len(starts), res), dtype=np.float64)
    for i, s in enumerate(starts):
        n = min(res, extent - s)
        out[i, :n] = share[i, s:s + n]
    return out


def load_volume(path):
    """Input volume as (D,H,W) float32.  .npz ('arr_0' or the first array) and .npy
    besides the reference's .tif/.tiff (tiff_io: tifffile when importable, else its own reader; scripts/test.py
    reads tif only, README.md:67 tells users to edit the loader for other formats)."""
    return _read_array(path).astype(np.float32)


def _read_array(path):
    """the (D,H,W) array of a volume file in the dtype it was stored in"""
    low = path.lower()
    if low.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            key = "arr_0" if "arr_0" in z.files else z.files[0]
            vol = z[key]
    elif low.endswith(".npy"):
        vol = np.load(path, allow_pickle=False)
    elif low.endswith((".tif", ".tiff")):
        from . import tiff_io
        vol = tiff_io.imread(path)
    else:
        raise ValueError("unsupported input file type: %s" % path)
    vol = np.asarray(vol)
    while vol.ndim > 3 and vol.shape[0] == 1:
        vol = vol[0]
    if vol.ndim != 3:
        raise ValueError("expected a (D,H,W) volume in %s, got %s" % (path, vol.shape))
    return vol


def load_labels(path):
    """Region labels as (D,H,W) int32 from the file types load_volume reads: 0 is unlabelled, every positive value
    names a region.  Values that are not integers, are negative or do not fit int32 are refused."""
    vol = _read_array(path)
    if vol.dtype.kind not in "iuf" or not np.all(np.isfinite(vol)) or np.any(vol != np.floor(vol)):
        raise ValueError("labels in %s are not integers (%s)" % (path, vol.dtype))
    if vol.size and (vol.min() < 0 or vol.max() > np.iinfo(np.int32).max):
        raise ValueError("labels in %s must lie in 0..2^31 - 1 (found %s..%s)" % (path, vol.min(), vol.max()))
    return vol.astype(np.int32)


# ---------------------------------------------------------------- joint patch sampling
class JointGeometry:
    """Canvas, patch starts and per-axis blend tables of one volume (joint_geometry)."""

    def __init__(self, canvas, res, x_starts, y_starts, z_starts, a_x, a_y, a_z, min_overlap=None):
        self.canvas, self.res = canvas, res
        self.min_overlap = min_overlap            # None: patch_grid's fixed grid; an integer: the sliding grid
        self.x_starts, self.y_starts, self.z_starts = x_starts, y_starts, z_starts
        self.a_x, self.a_y, self.a_z = a_x, a_y, a_z

    @property
    def n_patches(self):
        return len(self.x_starts) * len(self.y_starts) * len(self.z_starts)

    @property
    def grid(self):
        """[(x_start, y_start, z_start)] in patch_grid's order: p = (ix * ny + iy) * nz + iz."""
        return [(xs, ys, zs) for xs in self.x_starts for ys in self.y_starts for zs in self.z_starts]


def _axis_table(starts, extent, res, axis):
    """a[i][c]: patch i's share of coordinate c on one axis.  The Hann window over the Hann sum where that sum is
    positive; an equal share among the covering patches where it is 0 (np.hanning is 0 at both ends, so the
    outermost coordinate of an axis has no Hann weight at all)."""
    h = np.hanning(res)
    hann = np.zeros((len(starts), extent), dtype=np.float64)
    cover = np.zeros((len(starts), extent), dtype=bool)
    for i, s in enumerate(starts):
        if s < 0 or s >= extent:
            raise ValueError("axis %s: patch start %d outside 0..%d" % (axis, s, extent - 1))
        n = min(res, extent - s)
        hann[i, s:s + n] = h[:n]
        cover[i, s:s + n] = True
    count = cover.sum(axis=0)
    if (count == 0).any():
        raise ValueError("axis %s: coordinate %d of %d is covered by no patch (starts %s, patch size %d)"
                         % (axis, int(np.argmin(count > 0)), extent, list(starts), res))
    total = hann.sum(axis=0)
    live = total > 0
    table = np.where(live, hann / np.where(live, total, 1.0), cover / count)
    return table


def axis_cover(starts, extent, res):
    """(extent, 2) int32: per coordinate of one axis, {index of the first covering patch, number of covering
    patches}.  Ascending starts make the covering patches of a coordinate one run of indices (ddpm3d_tiling.d_cover:
    what ddpm3d_tiles_blend walks instead of all patches)."""
    starts = np.asarray(starts, dtype=np.int64)
    if starts.ndim != 1 or len(starts) < 1 or (np.diff(starts) <= 0).any():
        raise ValueError("axis_cover: starts must ascend, got %s" % (list(starts),))
    c = np.arange(extent)
    first = np.searchsorted(starts, c - res, side="right")       # first i with starts[i] + res > c
    end = np.searchsorted(starts, c, side="right")               # first i with starts[i] > c
    return np.stack([first, end - first], axis=1).astype(np.int32)


def joint_geometry(shape_dhw, res, num_xy=3, min_overlap=None):
    """Geometry of joint patch sampling for a (D, H, W) volume: the canvas (max(D, res), H, W), patch_grid's
    per-axis starts and the normalised blend weight as three fp64 tables,
    nw_p(z, x, y) = a_x[ix][x] * a_y[iy][y] * a_z[iz][z], which sum to 1 over the patches at every canvas voxel.
    With min_overlap (an integer in 2..res - 1) the starts are sliding_starts' on all three axes, for a volume of
    any size, and the canvas is max(extent, res) on every axis (num_xy is not used)."""
    D, H, W = (int(v) for v in shape_dhw)
    res = int(res)
    if min_overlap is not None:
        if res < 1 or min(D, H, W) < 1:
            raise ValueError("joint_geometry: bad shape (D=%d H=%d W=%d, patch size %d)" % (D, H, W, res))
        canvas = tuple(max(n, res) for n in (D, H, W))
        xs, ys, zs = (sliding_starts(n, res, min_overlap) for n in (H, W, D))
        return JointGeometry(canvas, res, xs, ys, zs, _axis_table(xs, canvas[1], res, "H"),
                             _axis_table(ys, canvas[2], res, "W"), _axis_table(zs, canvas[0], res, "D"),
                             min_overlap=int(min_overlap))
    if res < 1 or D < 1:
        raise ValueError("joint_geometry: bad shape (D=%d, patch size %d)" % (D, res))
    for axis, n in (("H", H), ("W", W)):
        if n < res:
            raise ValueError("axis %s: %d voxels is less than one patch of %d" % (axis, n, res))
    Dc = max(D, res)
    xs, ys, zs = xy_starts(H, res, num_xy), xy_starts(W, res, num_xy), z_starts(D, res)
    return JointGeometry((Dc, H, W), res, xs, ys, zs, _axis_table(xs, H, res, "H"), _axis_table(ys, W, res, "W"),
                         _axis_table(zs, Dc, res, "D"))


def joint_gather(canvas, geom):
    """(Dc, H, W) canvas -> (P, 1, res, res, res) patches in patch_grid's order (what ddpm3d_joint_gather copies)."""
    canvas = np.asarray(canvas)
    if canvas.shape != tuple(geom.canvas):
        raise ValueError("canvas of shape %s, geometry expects %s" % (canvas.shape, tuple(geom.canvas)))
    r = geom.res
    out = np.zeros((geom.n_patches, 1, r, r, r), dtype=canvas.dtype)
    for p, (xs, ys, zs) in enumerate(geom.grid):
        out[p, 0] = canvas[zs:zs + r, xs:xs + r, ys:ys + r]
    return out


def joint_blend(patch_values, geom):
    """(P, 1, res, res, res) float32 patches -> (Dc, H, W) float32 canvas: the normalised Hann blend of joint
    sampling.  This is the arithmetic ddpm3d_joint_blend reproduces bit for bit: per voxel, over the covering
    patches in ascending p, acc += float64(x_p) * ((a_x * a_y) * a_z) with the product and the sum rounded
    separately, then one rounding to float32."""
    patch_values = np.asarray(patch_values)
    r = geom.res
    if patch_values.shape != (geom.n_patches, 1, r, r, r):
        raise ValueError("patches of shape %s, geometry expects %s"
                         % (patch_values.shape, (geom.n_patches, 1, r, r, r)))
    acc = np.zeros(geom.canvas, dtype=np.float64)
    ny, nz = len(geom.y_starts), len(geom.z_starts)
    for p, (xs, ys, zs) in enumerate(geom.grid):
        ix, iy, iz = p // (ny * nz), (p // nz) % ny, p % nz
        w = (geom.a_x[ix][None, xs:xs + r, None] * geom.a_y[iy][None, None, ys:ys + r]) \
            * geom.a_z[iz][zs:zs + r, None, None]
        acc[zs:zs + r, xs:xs + r, ys:ys + r] += patch_values[p, 0].astype(np.float64) * w
    return acc.astype(np.float32)
