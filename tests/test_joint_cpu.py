"""
CPU tier of joint patch sampling: the per-axis blend tables of patches.joint_geometry are a
partition of unity built from the reference's Hann window, the numpy restatements joint_gather / joint_blend tile and
reassemble a canvas, the std attenuation of the one-shot blend that motivates the feature is what the issue states,
geometries the joint loop cannot serve are refused with the axis named, the two C entries are declared, exported
and bound within ABI 13 and refuse bad arguments on the host before any HIP call, and the inference script refuses
--joint_patches with --use_dpm_solver before any device call.  No GPU is touched here.
"""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT
from guided_diffusion import _hip, patches

GEOMETRIES = [(130, 200, 200, 96), (20, 40, 40, 16), (10, 40, 16, 16), (16, 40, 16, 16)]
FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_joint_gather", "ddpm3d_joint_blend")


def _axes(D, H, W, res):
    g = patches.joint_geometry((D, H, W), res)
    return g, [(g.a_x, g.x_starts, H), (g.a_y, g.y_starts, W), (g.a_z, g.z_starts, g.canvas[0])]


def _hann_rows(starts, extent, res):
    h = np.hanning(res)
    rows = np.zeros((len(starts), extent))
    for i, s in enumerate(starts):
        rows[i, s:s + res] = h
    return rows


@pytest.mark.parametrize("D,H,W,res", GEOMETRIES)
def test_tables_are_a_partition_of_unity_of_the_hann_window(D, H, W, res):
    g, axes = _axes(D, H, W, res)
    assert g.canvas == (max(D, res), H, W)
    assert g.grid == patches.patch_grid((D, H, W), res) and g.n_patches == len(g.grid)
    for table, starts, extent in axes:
        assert table.dtype == np.float64 and table.shape == (len(starts), extent)
        assert np.abs(table.sum(axis=0) - 1.0).max() <= 2 * np.finfo(np.float64).eps
        rows = _hann_rows(starts, extent, res)
        total = rows.sum(axis=0)
        equal_share = np.flatnonzero(total == 0)
        assert list(equal_share) == [0, extent - 1]            # np.hanning is 0 at both ends of the axis only
        for c in equal_share:
            cover = [i for i, s in enumerate(starts) if s <= c < s + res]
            assert cover and all(table[i, c] == 1.0 / len(cover) for i in cover)
            assert all(table[i, c] == 0 for i in range(len(starts)) if i not in cover)
        live = total > 0
        np.testing.assert_allclose((table * total)[:, live], rows[:, live], rtol=4 * np.finfo(np.float64).eps,
                                   atol=0)


@pytest.mark.parametrize("D,H,W,res", GEOMETRIES)
def test_hann_sums_match_the_one_shot_stitcher_weight(D, H, W, res):
    g, axes = _axes(D, H, W, res)
    sx, sy, sz = (_hann_rows(starts, extent, res).sum(axis=0) for _, starts, extent in axes)
    h = np.hanning(res)
    norm = np.outer(np.outer(h, h).ravel(), h).max()         # hann_window_3d's normaliser
    want = (sx[:, None, None] * sy[None, :, None] * sz[None, None, :D]) / norm      # (H, W, Z)
    ones = [np.ones((res, res, res), dtype=np.float32)] * g.n_patches
    _, weight = patches.stitch_patches(ones, g.grid, (D, H, W), res)
    live = want > 0
    assert np.array_equal(weight > 0, live)
    rel = np.abs(weight[live] - want[live]) / want[live]
    print("stitcher weight vs product of per-axis Hann sums: max rel %.3g" % rel.max())
    assert rel.max() < 1e-6


@pytest.mark.parametrize("D,H,W,res", GEOMETRIES)
def test_gather_is_split_volume_and_blend_inverts_it(D, H, W, res):
    g = patches.joint_geometry((D, H, W), res)
    rng = np.random.default_rng(D * 1000 + res)
    vol = rng.standard_normal((D, H, W)).astype(np.float32)
    canvas = np.zeros(g.canvas, dtype=np.float32)
    canvas[:D] = vol
    tiles = patches.joint_gather(canvas, g)
    want, grid = patches.split_volume(vol, res)
    assert grid == g.grid and tiles.dtype == np.float32 and np.array_equal(tiles, want)
    # partition of unity: blending the tiles of a canvas returns the canvas
    canvas = rng.standard_normal(g.canvas).astype(np.float32)
    back = patches.joint_blend(patches.joint_gather(canvas, g), g)
    assert back.dtype == np.float32 and back.shape == g.canvas
    assert np.all(np.abs(back - canvas) <= np.spacing(np.abs(canvas)))


@pytest.mark.parametrize("D,H,W,res", [(20, 40, 40, 16), (16, 40, 16, 16), (20, 40, 44, 16)])
def test_blend_of_disagreeing_patches_is_the_reference_blend(D, H, W, res):
    """joint_blend of patches that disagree in overlaps equals the reference's one-shot Hann blend
    (patches.stitch_patches) wherever that blend has weight: the same weights per patch, so a_x / a_y / a_z cannot be
    mixed up.  Bound: stitch_patches rounds its fp32 accumulator after each of at most 8 terms and divides once, each
    rounding at most 2^-24 of a partial sum that is at most max|x| times the weight sum; joint_blend rounds once.
    16 * 2^-24 * max|x| covers the ten roundings with room for the fp32 weight sum's own."""
    g = patches.joint_geometry((D, H, W), res)
    assert g.canvas == (D, H, W)                               # no depth extension in these cases
    rng = np.random.default_rng(H + W)
    tiles = rng.standard_normal((g.n_patches, 1, res, res, res)).astype(np.float32)
    got = patches.joint_blend(tiles, g)                        # (D, H, W)
    want, weight = patches.stitch_patches([t[0].transpose(1, 2, 0) for t in tiles], g.grid, (D, H, W), res)
    live = weight > 0                                          # (H, W, Z)
    err = np.abs(got.transpose(1, 2, 0) - want)[live].max()
    print("joint_blend vs stitch_patches on %d voxels of non-zero weight: max abs %.3g" % (live.sum(), err))
    assert live.sum() > 0.7 * live.size and err <= 16 * 2.0 ** -24 * np.abs(tiles).max()


def test_one_shot_blend_attenuates_the_std_as_the_issue_states():
    """std of a Hann blend of independent draws over the true std, sqrt(sum w^2) / sum w, for 200x200x130 / 96."""
    D, H, W, res = 130, 200, 200, 96
    win = patches.hann_window_3d(res)
    s1, s2, n = np.zeros((H, W, D)), np.zeros((H, W, D)), np.zeros((H, W, D), dtype=np.int64)
    for xs, ys, zs in patches.patch_grid((D, H, W), res):
        s1[xs:xs + res, ys:ys + res, zs:zs + res] += win
        s2[xs:xs + res, ys:ys + res, zs:zs + res] += win * win
        n[xs:xs + res, ys:ys + res, zs:zs + res] += 1
    live = s1 > 0
    f = np.sqrt(s2[live]) / s1[live]
    assert [int((n == k).sum()) for k in (1, 2, 4, 8)] == [852992, 2118144, 1748736, 480128]     # all voxels
    assert n.min() == 1 and round(float(f.min()), 3) == 0.354 == round(1 / np.sqrt(8), 3)
    assert round(float(np.median(f)), 3) == 0.822
    assert round(float((f < 0.9).mean()), 2) == 0.62 and round(float((f < 0.75).mean()), 2) == 0.38


@pytest.mark.parametrize("shape,res,num_xy,axis", [
    ((130, 90, 200), 96, 3, "H"), ((130, 200, 95), 96, 3, "W"),           # less than one patch
    ((193, 200, 200), 96, 3, "D"), ((130, 289, 200), 96, 3, "H"), ((130, 200, 400), 96, 3, "W"),   # a gap
    ((20, 40, 40), 16, 2, "H"),
])
def test_geometry_refuses_what_it_cannot_tile(shape, res, num_xy, axis):
    with pytest.raises(ValueError, match=r"axis %s\b" % axis):
        patches.joint_geometry(shape, res, num_xy)


def test_geometry_accepts_the_edges_of_what_it_can_tile():
    assert patches.joint_geometry((192, 288, 96), 96).canvas == (192, 288, 96)
    assert patches.joint_geometry((1, 16, 16), 16).canvas == (16, 16, 16)


def test_restatements_refuse_mismatched_shapes():
    g = patches.joint_geometry((20, 40, 40), 16)
    with pytest.raises(ValueError):
        patches.joint_gather(np.zeros((20, 40, 41), dtype=np.float32), g)
    with pytest.raises(ValueError):
        patches.joint_blend(np.zeros((17, 1, 16, 16, 16), dtype=np.float32), g)


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_JOINT_MAX_STARTS %d\b" % _hip.JOINT_MAX_STARTS, hdr)
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    assert ctypes.sizeof(_hip.JointStarts) == 4 * (3 + 3 * _hip.JOINT_MAX_STARTS)


def starts_struct(xs, ys, zs):
    s = _hip.JointStarts()
    s.nx, s.ny, s.nz = len(xs), len(ys), len(zs)
    for arr, vals in ((s.xs, xs), (s.ys, ys), (s.zs, zs)):
        for i, v in enumerate(vals[:_hip.JOINT_MAX_STARTS]):
            arr[i] = v
    return s


# what both entries refuse: (argument overrides, start-list overrides)
BAD_COMMON = [
    (dict(B=0), {}), (dict(B=-1), {}), (dict(B=65), {}),
    (dict(res=0), {}), (dict(res=-16), {}), (dict(res=1025), {}),
    (dict(Dc=0), {}), (dict(H=-1), {}), (dict(W=0), {}), (dict(Dc=65536), {}), (dict(H=65536), {}),
    (dict(W=1 << 30), {}), (dict(H=65534, W=32769), {}),      # a plane that 32-bit thread indices cannot round up
    # a patch that leaves the canvas: start + res > extent
    ({}, dict(xs=[0, 12, 25])), ({}, dict(ys=[0, 12, 39])), ({}, dict(zs=[0, 5])), (dict(Dc=15), dict(zs=[0])),
    ({}, dict(xs=list(range(9)))), ({}, dict(ys=[0] * 9)), ({}, dict(zs=[0] * 9)), ({}, dict(xs=[])),
    ({}, dict(xs=[0, 12, 40])), ({}, dict(ys=[-1, 12, 24])), ({}, dict(zs=[0, 20])), ({}, dict(zs=[-4, 4])),
]


def _call(name, over, sover, **extra):
    st = dict(xs=[0, 12, 24], ys=[0, 12, 24], zs=[0, 4])
    st.update(sover)
    s = starts_struct(**st)
    s.nx, s.ny, s.nz = len(st["xs"]), len(st["ys"]), len(st["zs"])           # counts above the array size included
    a = dict(src=FAKE, B=2, Dc=20, H=40, W=40, res=16, starts=ctypes.byref(s))
    a.update(extra)
    a.update(over)
    lib = _hip.load()
    rc = getattr(lib, name)(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


@pytest.mark.parametrize("over,sover", BAD_COMMON + [
    (dict(src=None), {}), (dict(out=None), {}), (dict(starts=None), {}),
    (dict(first_patch=-1), {}), (dict(n_patches=0), {}), (dict(first_patch=17, n_patches=2), {}),
    (dict(first_patch=18, n_patches=1), {}), (dict(n_patches=19), {}),
    (dict(first_patch=1 << 30, n_patches=1 << 30), {}),
])
def test_joint_gather_refuses_bad_arguments(over, sover):
    rc, msg = _call("ddpm3d_joint_gather", over, sover, first_patch=0, n_patches=18, out=FAKE, stream=None)
    assert rc == _hip.E_INVAL and msg.startswith("joint_gather:"), (rc, msg)


@pytest.mark.parametrize("over,sover", BAD_COMMON + [
    (dict(src=None), {}), (dict(tables=None), {}), (dict(out=None), {}), (dict(starts=None), {}),
    # an axis with a coordinate no patch covers
    ({}, dict(xs=[0, 24])), ({}, dict(ys=[1, 12, 24])), ({}, dict(zs=[0])), ({}, dict(zs=[3, 4])),
    (dict(H=57), {}), (dict(Dc=40), {}),
])
def test_joint_blend_refuses_bad_arguments(over, sover):
    rc, msg = _call("ddpm3d_joint_blend", over, sover, tables=FAKE, out=FAKE, stream=None)
    assert rc == _hip.E_INVAL and msg.startswith("joint_blend:"), (rc, msg)


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_refuses_joint_dpm_solver_before_any_device_call(tmp_path, monkeypatch, capsys):
    mod = _script()

    def no_device(*a, **kw):
        raise AssertionError("the script went past its argument checks")

    monkeypatch.setattr(mod, "sr_create_model_and_diffusion", no_device)
    monkeypatch.setattr(mod.dist_util, "setup_dist", no_device)
    with pytest.raises(SystemExit) as e:
        mod.main(["--joint_patches", "True", "--use_dpm_solver", "True", "--base_samples",
                  str(tmp_path / "none.npz"), "--save_dir", str(tmp_path)])
    assert e.value.code == 2
    assert "--joint_patches" in capsys.readouterr().err


def test_script_defaults_to_independent_patches():
    assert _script().create_argparser().parse_args([]).joint_patches is False


def test_joint_loop_refuses_the_dpm_solver():
    from guided_diffusion import joint
    g = patches.joint_geometry((20, 40, 40), 16)
    with pytest.raises(ValueError, match="DPM-Solver"):
        next(joint.sample_loop_progressive(None, None, np.zeros((20, 40, 40), np.float32), g, kind="dpm_solver"))
