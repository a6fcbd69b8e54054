"""
CPU tier of the gap-free sliding tiling: patches.sliding_starts has the properties the design rests
on for every legal overlap (first and last start, strict ascent, the minimum overlap, a positive Hann sum everywhere
but the two ends of the axis), the grid is the reference's own for the reference's volumes, joint_geometry's sliding
form is a partition of unity on volumes the fixed grid cannot tile and leaves the default form as it was, the one-shot
stitcher has weight 0 on the six faces only, the two C entries are declared, exported and bound within ABI 13 and
refuse bad arguments on the host before any HIP call, and the script refuses a bad --patch_overlap before any device
call.  No GPU is touched here.
"""

import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT
from guided_diffusion import _hip, patches

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first


@pytest.mark.parametrize("res", [8, 16, 32, 96])
def test_sliding_starts_properties_exhaustively(res):
    """Every legal overlap and every extent in 1..419."""
    h = np.hanning(res)
    for ov in range(2, res):
        for extent in range(1, 420):
            s = patches.sliding_starts(extent, res, ov)
            if extent <= res:
                assert s == [0]
                continue
            n = -(-(extent - res) // (res - ov)) + 1
            assert len(s) == n and s == [(i * (extent - res)) // (n - 1) for i in range(n)]
            assert s[0] == 0 and s[-1] == extent - res
            d = np.diff(s)
            assert d.min() >= 1 and res - d.max() >= ov, (extent, res, ov, s)
            total = np.zeros(extent)
            for a in s:
                total[a:a + res] += h
            assert total[0] == 0 and total[-1] == 0 and total[1:-1].min() > 0, (extent, res, ov, s)


def test_overlaps_below_two_can_leave_interior_planes_without_weight():
    """Why 0 and 1 are refused: the same formula with those overlaps has a zero Hann sum inside the axis."""
    h = np.hanning(16)
    for ov, extent in ((0, 32), (1, 31)):
        n = -(-(extent - 16) // (16 - ov)) + 1
        total = np.zeros(extent)
        for i in range(n):
            a = (i * (extent - 16)) // (n - 1)
            total[a:a + 16] += h
        assert (total[1:-1] == 0).any()


@pytest.mark.parametrize("ov,res", [(0, 16), (1, 16), (16, 16), (17, 16), (-1, 16), (96, 96), (2, 2)])
def test_sliding_starts_refuses_bad_overlaps(ov, res):
    with pytest.raises(ValueError, match="overlap"):
        patches.sliding_starts(100, res, ov)
    with pytest.raises(ValueError, match="overlap"):
        patches.sliding_grid((100, 100, 100), res, ov)
    with pytest.raises(ValueError, match="overlap"):
        patches.joint_geometry((100, 100, 100), res, min_overlap=ov)


def test_sliding_grid_is_the_references_grid_on_the_references_volumes():
    for D in range(90, 131):
        assert patches.sliding_grid((D, 200, 200), 96, 44) == patches.patch_grid((D, 200, 200), 96), D
    assert patches.sliding_grid((24, 40, 40), 16, 4) == patches.patch_grid((24, 40, 40), 16)


def test_patch_counts_of_a_whole_body_volume():
    for ov, count in ((44, 8 * 8 * 13), (32, 539), (16, 324)):
        assert len(patches.sliding_grid((700, 440, 440), 96, ov)) == count


SLIDING = [((40, 70, 52), 16, 4), ((10, 70, 12), 16, 4), ((24, 40, 40), 16, 4), ((130, 200, 200), 96, 44),
           ((30, 100, 33), 16, 7), ((5, 7, 9), 16, 2)]


@pytest.mark.parametrize("shape,res,ov", SLIDING)
def test_sliding_geometry_is_a_partition_of_unity(shape, res, ov):
    g = patches.joint_geometry(shape, res, min_overlap=ov)
    D, H, W = shape
    assert g.canvas == (max(D, res), max(H, res), max(W, res)) and g.min_overlap == ov
    assert g.grid == patches.sliding_grid(shape, res, ov) and g.n_patches == len(g.grid)
    for table, starts, extent in ((g.a_x, g.x_starts, g.canvas[1]), (g.a_y, g.y_starts, g.canvas[2]),
                                  (g.a_z, g.z_starts, g.canvas[0])):
        assert table.dtype == np.float64 and table.shape == (len(starts), extent)
        assert np.abs(table.sum(axis=0) - 1.0).max() <= 2 * np.finfo(np.float64).eps
    # the weights sum to 1 at every canvas voxel
    total = np.zeros(g.canvas)
    ny, nz = len(g.y_starts), len(g.z_starts)
    for p, (xs, ys, zs) in enumerate(g.grid):
        ix, iy, iz = p // (ny * nz), (p // nz) % ny, p % nz
        total[zs:zs + res, xs:xs + res, ys:ys + res] += (
            g.a_x[ix][None, xs:xs + res, None] * g.a_y[iy][None, None, ys:ys + res]
            * g.a_z[iz][zs:zs + res, None, None])
    assert np.abs(total - 1.0).max() <= 8 * np.finfo(np.float64).eps
    # and blending the tiles of a canvas returns the canvas
    canvas = np.random.default_rng(D).standard_normal(g.canvas).astype(np.float32)
    back = patches.joint_blend(patches.joint_gather(canvas, g), g)
    assert np.all(np.abs(back - canvas) <= np.spacing(np.abs(canvas)))


def test_sliding_geometry_accepts_what_the_fixed_grid_refuses():
    for shape in ((40, 70, 52), (10, 70, 12)):
        with pytest.raises(ValueError):
            patches.joint_geometry(shape, 16)
        g = patches.joint_geometry(shape, 16, min_overlap=4)
        assert len(g.x_starts) == 6 and g.x_starts[-1] == 70 - 16
    g = patches.joint_geometry((10, 70, 12), 16, min_overlap=4)
    assert g.canvas == (16, 70, 16) and g.y_starts == [0] and g.z_starts == [0]


def test_default_geometry_is_unchanged():
    """Without min_overlap: patch_grid's starts, the (max(D, res), H, W) canvas, the same fields on every call, and
    the refusals with the messages in the code."""
    for shape, res in (((130, 200, 200), 96), ((20, 40, 40), 16), ((10, 40, 16), 16)):
        a, b = patches.joint_geometry(shape, res), patches.joint_geometry(shape, res, 3, None)
        assert a.min_overlap is None and b.min_overlap is None
        assert a.canvas == b.canvas == (max(shape[0], res), shape[1], shape[2]) and a.res == b.res == res
        assert a.grid == b.grid == patches.patch_grid(shape, res)
        assert (a.x_starts, a.y_starts, a.z_starts) == (patches.xy_starts(shape[1], res), patches.xy_starts(shape[2], res),
                                                        patches.z_starts(shape[0], res))
        for t, u in ((a.a_x, b.a_x), (a.a_y, b.a_y), (a.a_z, b.a_z)):
            assert np.array_equal(t, u)
    with pytest.raises(ValueError, match=r"axis H: 90 voxels is less than one patch of 96"):
        patches.joint_geometry((130, 90, 200), 96)
    with pytest.raises(ValueError, match=r"axis W: 95 voxels is less than one patch of 96"):
        patches.joint_geometry((130, 200, 95), 96)
    with pytest.raises(ValueError, match=r"axis D: coordinate 96 of 193 is covered by no patch"):
        patches.joint_geometry((193, 200, 200), 96)
    with pytest.raises(ValueError, match=r"joint_geometry: bad shape \(D=0, patch size 16\)"):
        patches.joint_geometry((0, 40, 40), 16)


@pytest.mark.parametrize("shape,res,ov", [((40, 70, 52), 16, 4), ((24, 40, 40), 16, 2), ((50, 33, 90), 16, 9)])
def test_one_shot_stitcher_on_a_sliding_grid_has_weight_zero_on_the_six_faces_only(shape, res, ov):
    D, H, W = shape
    grid = patches.sliding_grid(shape, res, ov)
    ones = [np.ones((res, res, res), dtype=np.float32)] * len(grid)
    out, weight = patches.stitch_patches(ones, grid, shape, res)              # (H, W, Z)
    faces = np.zeros((H, W, D), dtype=bool)
    faces[0] = faces[-1] = faces[:, 0] = faces[:, -1] = True
    faces[:, :, 0] = faces[:, :, -1] = True
    assert np.array_equal(weight == 0, faces)
    assert np.all(out[faces] == 0) and np.allclose(out[~faces], 1.0, rtol=1e-5)


def test_grid_gaps_names_the_axes_the_fixed_grid_leaves_open():
    assert patches.grid_gaps((130, 200, 200), 96) == {"D": 0, "H": 0, "W": 0}
    assert patches.grid_gaps((20, 40, 40), 16) == {"D": 0, "H": 0, "W": 0}
    assert patches.grid_gaps((10, 16, 16), 16) == {"D": 0, "H": 0, "W": 0}
    # 440 wide: starts [0, 172, 344]; 700 deep: [0, 604]
    assert patches.grid_gaps((700, 440, 440), 96) == {"D": 700 - 192, "H": 440 - 288, "W": 440 - 288}
    assert patches.grid_gaps((16, 60, 16), 16) == {"D": 0, "H": 12, "W": 0}


@pytest.mark.parametrize("starts,extent,res", [([0], 16, 16), ([0, 12, 24], 40, 16), ([0, 1, 2, 3, 19], 35, 16),
                                                (patches.sliding_starts(440, 96, 44), 440, 96)])
def test_axis_cover_is_the_run_of_covering_patches(starts, extent, res):
    cover = patches.axis_cover(starts, extent, res)
    assert cover.dtype == np.int32 and cover.shape == (extent, 2)
    for c in range(extent):
        want = [i for i, s in enumerate(starts) if s <= c < s + res]
        assert want and list(range(cover[c, 0], cover[c, 0] + cover[c, 1])) == want
    with pytest.raises(ValueError):
        patches.axis_cover([0, 12, 12], 40, 16)


ENTRIES = ("ddpm3d_tiles_gather", "ddpm3d_tiles_blend")


def test_entries_are_declared_exported_and_bound_within_abi_13():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert "typedef struct ddpm3d_tiling" in hdr
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_hip.Tiling) == 16 + 6 * p          # int32[3] padded to a pointer, then six pointers


def tiling(xs, ys, zs, counts=None, **over):
    """A descriptor on host starts with FAKE device tables; returns (struct, keep-alive)."""
    t = _hip.Tiling()
    keep = []
    for a, vals in enumerate((xs, ys, zs)):
        arr = (ctypes.c_int32 * max(len(vals), 1))(*vals)
        keep.append(arr)
        t.n[a] = len(vals) if counts is None else counts[a]
        t.starts[a] = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))
    t.d_starts, t.d_cover, t.d_tables = FAKE, FAKE, FAKE
    for k, v in over.items():
        if k == "null_axis":
            t.starts[v] = ctypes.POINTER(ctypes.c_int32)()
        else:
            setattr(t, k, v)
    return t, keep


# what both entries refuse: (argument overrides, descriptor overrides)
BAD_COMMON = [
    (dict(B=0), {}), (dict(B=-1), {}), (dict(B=65), {}),
    (dict(res=0), {}), (dict(res=-16), {}), (dict(res=1025), {}),
    (dict(Dc=0), {}), (dict(H=-1), {}), (dict(W=0), {}), (dict(Dc=65536), {}), (dict(H=65536), {}),
    (dict(W=1 << 30), {}), (dict(H=65534, W=32769), {}),
    # a patch that leaves the canvas
    ({}, dict(xs=[0, 12, 25])), ({}, dict(ys=[0, 12, 39])), ({}, dict(zs=[0, 5])), (dict(Dc=15), dict(zs=[0])),
    ({}, dict(xs=[0, 12, 40])), ({}, dict(ys=[-1, 12, 24])), ({}, dict(zs=[-4, 4])),
    # no start, a NULL start list, starts that do not ascend, more starts than coordinates
    ({}, dict(xs=[])), ({}, dict(null_axis=1)), ({}, dict(ys=[0, 24, 12])), ({}, dict(zs=[0, 0, 4])),
    ({}, dict(xs=[0, 12, 24], counts=(41, 3, 2))), ({}, dict(xs=[0, 12, 24], counts=(-1, 3, 2))),
    ({}, dict(d_starts=None)),
]


def _call(name, over, tover, **extra):
    st = dict(xs=[0, 12, 24], ys=[0, 12, 24], zs=[0, 4])
    st.update(tover)
    t, keep = tiling(**st)
    a = dict(src=FAKE, B=2, Dc=20, H=40, W=40, res=16, tiling=ctypes.byref(t))
    a.update(extra)
    a.update(over)
    lib = _hip.load()
    rc = getattr(lib, name)(*a.values())
    del keep
    return rc, lib.ddpm3d_last_error().decode()


@pytest.mark.parametrize("over,tover", BAD_COMMON + [
    (dict(src=None), {}), (dict(out=None), {}), (dict(tiling=None), {}),
    (dict(first_patch=-1), {}), (dict(n_patches=0), {}), (dict(first_patch=17, n_patches=2), {}),
    (dict(first_patch=18, n_patches=1), {}), (dict(n_patches=19), {}),
    (dict(first_patch=1 << 30, n_patches=1 << 30), {}),
])
def test_tiles_gather_refuses_bad_arguments(over, tover):
    rc, msg = _call("ddpm3d_tiles_gather", over, tover, first_patch=0, n_patches=18, out=FAKE, stream=None)
    assert rc == _hip.E_INVAL and msg.startswith("tiles_gather:"), (rc, msg)


@pytest.mark.parametrize("over,tover", BAD_COMMON + [
    (dict(src=None), {}), (dict(out=None), {}), (dict(tiling=None), {}),
    ({}, dict(d_cover=None)), ({}, dict(d_tables=None)), ({}, dict(d_cover=FAKE + 4)),
    # an axis with a coordinate no patch covers
    ({}, dict(xs=[0, 24])), ({}, dict(ys=[1, 12, 24])), ({}, dict(zs=[0])), ({}, dict(zs=[3, 4])),
    (dict(H=57), {}), (dict(Dc=40), {}),
])
def test_tiles_blend_refuses_bad_arguments(over, tover):
    rc, msg = _call("ddpm3d_tiles_blend", over, tover, out=FAKE, stream=None)
    assert rc == _hip.E_INVAL and msg.startswith("tiles_blend:"), (rc, msg)


def test_entries_refuse_more_rows_than_they_can_index():
    """P * B above 2^31 - 1 rows: 1291 starts on each axis of a 1306^3 canvas (res 16, stride 1) are 2.15e9 patches."""
    starts = list(range(1291))
    t, keep = tiling(starts, starts, starts)
    lib = _hip.load()
    rc = lib.ddpm3d_tiles_blend(FAKE, 1, 1306, 1306, 1306, 16, ctypes.byref(t), FAKE, None)
    assert rc == _hip.E_INVAL and "too many rows" in lib.ddpm3d_last_error().decode()
    rc = lib.ddpm3d_tiles_gather(FAKE, 1, 1306, 1306, 1306, 16, ctypes.byref(t), 0, 1, FAKE, None)
    assert rc == _hip.E_INVAL and "too many rows" in lib.ddpm3d_last_error().decode()


def test_more_than_eight_starts_pass_validation_up_to_the_patch_range():
    """No compile-time limit on the starts per axis: ten starts along H are accepted (the call is then refused for
    its patch range, the last check before a launch)."""
    xs = patches.sliding_starts(70, 16, 10)
    assert len(xs) == 10
    t, keep = tiling(xs, [0, 12, 24], [0, 4])
    lib = _hip.load()
    rc = lib.ddpm3d_tiles_gather(FAKE, 1, 20, 70, 40, 16, ctypes.byref(t), 60, 1, FAKE, None)
    assert rc == _hip.E_INVAL and lib.ddpm3d_last_error().decode() == "tiles_gather: patches 60..60 of 60"


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("ov", ["0", "1", "16", "-2", "40"])
def test_script_refuses_a_bad_patch_overlap_before_any_device_call(tmp_path, monkeypatch, capsys, ov):
    mod = _script()

    def no_device(*a, **kw):
        raise AssertionError("the script went past its argument checks")

    monkeypatch.setattr(mod, "sr_create_model_and_diffusion", no_device)
    monkeypatch.setattr(mod.dist_util, "setup_dist", no_device)
    monkeypatch.setattr(mod.patches, "load_volume", no_device)
    with pytest.raises(SystemExit) as e:
        mod.main(["--patch_overlap", ov, "--large_size", "16", "--small_size", "16", "--base_samples",
                  str(tmp_path / "none.npz"), "--save_dir", str(tmp_path)])
    assert e.value.code == 2
    assert "--patch_overlap" in capsys.readouterr().err


def test_script_defaults_to_the_fixed_grid():
    assert _script().create_argparser().parse_args([]).patch_overlap == -1


def test_volume_stitcher_takes_one_draw_and_draw_stitcher_still_refuses_it():
    from guided_diffusion import uncertainty
    assert issubclass(uncertainty.DrawStitcher, uncertainty.VolumeStitcher)
    for K in (1, 0, 65, 2.0):
        with pytest.raises(ValueError, match="DrawStitcher: needs 2..64 draws"):
            uncertainty.DrawStitcher((16, 16, 16), 16, K, "cpu")
    for K in (0, 65):
        with pytest.raises(ValueError, match="VolumeStitcher: needs 1..64 draws"):
            uncertainty.VolumeStitcher((16, 16, 16), 16, K, "cpu")
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        uncertainty.VolumeStitcher((16, 16, 16), 16, 1, "cpu")


def test_built_library_passes_the_store_hazard_check():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_store_hazard.py")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
