"""
CPU tier of the lesion segmentation: the yardstick of tests/segment_ref.py on hand-made cases whose
answer is written out, the two C entries declared, exported and bound within ABI 13, every host refusal of the entry
(no HIP call is made: the pointers are fake), the workspace query, and the inference script's refusals of bad
--roi_threshold / --roi_threshold_frac / --roi_connectivity / --roi_min_voxels before any device call.  No GPU is
touched here.
"""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import segment_ref as S
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics, patches

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_label_components", "ddpm3d_label_components_workspace_bytes")
ONE_SHORT = "one byte less than the entry's own answer"


# ------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_corner_and_edge_pairs():
    corner = np.zeros((3, 3, 3), dtype=bool)
    corner[0, 0, 0] = corner[1, 1, 1] = True
    assert [S.label(corner, c)[1] for c in (26, 18, 6)] == [1, 2, 2]
    edge = np.zeros((3, 3, 3), dtype=bool)
    edge[0, 1, 1] = edge[1, 2, 1] = True
    assert [S.label(edge, c)[1] for c in (26, 18, 6)] == [1, 1, 2]
    face = np.zeros((3, 3, 3), dtype=bool)
    face[1, 1, 1] = face[1, 1, 2] = True
    assert [S.label(face, c)[1] for c in (26, 18, 6)] == [1, 1, 1]


def test_yardstick_numbers_in_raster_order_and_gives_roots():
    m = np.zeros((2, 3, 4), dtype=bool)
    m[0, 0, 3] = m[0, 1, 3] = True                       # first voxel at flat index 3
    m[0, 2, 0] = True                                    # first voxel at 8
    m[1, 0, 0] = m[1, 0, 1] = True                       # first voxel at 12
    labels, n = S.label(m, 6)
    assert n == 3 and labels[0, 0, 3] == labels[0, 1, 3] == 1 and labels[0, 2, 0] == 2 and labels[1, 0, 1] == 3
    roots = S.roots(labels)
    assert roots.dtype == np.int32 and roots[0, 1, 3] == 3 and roots[0, 2, 0] == 8 and roots[1, 0, 1] == 12
    assert (roots[~m] == -1).all()
    assert S.roots(np.zeros((2, 2, 2), dtype=np.int32)).tolist() == [[[-1, -1]] * 2] * 2


def test_yardstick_foreground_threshold_nan_and_keep():
    v = np.array([[[1.0, 2.0, np.nan, 2.5, 3.0]]], dtype=np.float32)
    assert S.foreground(v, 2.0).tolist() == [[[False, False, False, True, True]]]
    keep = np.array([[[1, 1, 1, 0, 7]]], dtype=np.uint8)
    assert S.foreground(v, 2.0, keep).tolist() == [[[False, False, False, False, True]]]


def test_yardstick_segment_filters_and_renumbers():
    v = np.zeros((1, 3, 8), dtype=np.float32)
    v[0, 0, 0] = 1                                       # 1 voxel
    v[0, 0, 2:5] = 1                                     # 3 voxels
    v[0, 2, 0:2] = 1                                     # 2 voxels
    v[0, 2, 4:8] = 1                                     # 4 voxels
    labels, n = S.segment(v, 0.5, 6, 1)
    assert n == 4 and labels[0].tolist() == [[1, 0, 2, 2, 2, 0, 0, 0], [0] * 8, [3, 3, 0, 0, 4, 4, 4, 4]]
    labels, n = S.segment(v, 0.5, 6, 2)
    assert n == 3 and labels[0].tolist() == [[0, 0, 1, 1, 1, 0, 0, 0], [0] * 8, [2, 2, 0, 0, 3, 3, 3, 3]]
    labels, n = S.segment(v, 0.5, 6, 4)
    assert n == 1 and labels[0, 2].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and labels.dtype == np.int32
    assert S.segment(v, 0.5, 6, 5)[1] == 0


def test_yardstick_detection_on_the_blob_pair():
    t, e = S.blobs_pair()
    tl, nt = S.segment(t, 1.0)
    el, ne = S.segment(e, 1.0)
    assert (nt, ne) == (5, 7)
    d = S.detection(tl, el)
    assert d["found"] == [False, True, True, True, True] and d["overlap"] == [0, 8, 96, 96, 180]
    assert (d["n_found"], d["n_missed"], d["false_positives"], d["sensitivity"]) == (4, 1, 2, 0.8)
    none = S.detection(np.zeros_like(tl), el)
    assert none["sensitivity"] is None and none["false_positives"] == 7 and none["found"] == []


def test_yardstick_shapes_of_the_gpu_tier():
    for shape in ((19, 17, 133), (1, 1, 5), (3, 1, 1)):
        assert [S.label(S.serpentine(shape), c)[1] for c in (6, 18, 26)] == [1, 1, 1]
    board = S.checkerboard((5, 4, 7))
    assert [S.label(board, c)[1] for c in (6, 18, 26)] == [int(board.sum()), 1, 1]


def test_blend_cover_is_the_stitcher_s_positive_weight():
    shape, res = (20, 40, 40), 16
    grid = patches.patch_grid(shape, res)
    ones = [np.ones((res, res, res), dtype=np.float32)] * len(grid)
    _, weight = patches.stitch_patches(ones, grid, shape, res)
    cover = patches.blend_cover(grid, shape, res)
    assert cover.shape == weight.shape and cover.dtype == bool and np.array_equal(cover, weight > 0)
    assert not cover[0].any() and not cover[:, -1].any() and not cover[:, :, 0].any() and cover[1:-1, 1:-1, 1:-1].all()
    grid = patches.sliding_grid((20, 37, 45), res, 4)
    ones = [np.ones((res, res, res), dtype=np.float32)] * len(grid)
    _, weight = patches.stitch_patches(ones, grid, (20, 37, 45), res)
    assert np.array_equal(patches.blend_cover(grid, (20, 37, 45), res), weight > 0)


# ------------------------------------------------------------------------------------------ the C entries
def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    tile = tuple(int(re.search(r"#define DDPM3D_CCL_TILE_%s (\d+)\b" % a, hdr).group(1)) for a in "DHW")
    assert tile == _hip.CCL_TILE and tile[2] % 64 == 0 and all(v >= 1 for v in tile)
    assert 4 * (tile[0] + 2) * (tile[1] + 2) * (tile[2] + 2) <= 32 * 1024       # labels and halo: well under 64 KB
    assert "ccl.o" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert os.path.isfile(os.path.join(PKG, "csrc", "ccl.hip"))


def _label(**over):
    lib = _hip.load()
    a = dict(vol=FAKE, keep=None, threshold=0.5, connectivity=26, D=20, H=30, W=40, roots=FAKE, ws=FAKE,
             ws_bytes=1 << 30, status=FAKE, stream=None)
    a.update(over)
    if a["ws_bytes"] == ONE_SHORT:
        a["ws_bytes"] = lib.ddpm3d_label_components_workspace_bytes(a["D"], a["H"], a["W"]) - 1
        assert a["ws_bytes"] > 0
    rc = lib.ddpm3d_label_components(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(vol=None), dict(roots=None), dict(status=None), dict(ws=None),
    dict(connectivity=0), dict(connectivity=4), dict(connectivity=8), dict(connectivity=27), dict(connectivity=-6),
    dict(D=0), dict(H=0), dict(W=0), dict(D=-1), dict(W=-64),
    dict(D=1 << 11, H=1 << 10, W=1 << 10), dict(D=1, H=1 << 16, W=1 << 16), dict(D=46341, H=46341, W=1),
    dict(threshold=float("nan")),
    dict(ws_bytes=0), dict(ws_bytes=ONE_SHORT), dict(ws=FAKE + 8), dict(ws=FAKE + 4),
], ids=lambda o: "-".join("%s=%s" % kv for kv in o.items())[:40])
def test_label_components_refuses_bad_arguments(over):
    rc, msg = _label(**over)
    assert rc == _hip.E_INVAL and msg.startswith("label_components:"), (rc, msg)


def test_workspace_sizes():
    ws = _hip.load().ddpm3d_label_components_workspace_bytes
    for shape in ((1, 1, 1), (20, 30, 40), (130, 200, 200), (700, 440, 440), (1, 1, (1 << 31) - 1),
                  ((1 << 31) - 1, 1, 1)):
        need = ws(*shape)
        voxels = shape[0] * shape[1] * shape[2]
        assert need >= 16 and need % 16 == 0, shape
        assert need <= 64 + voxels * 4, shape             # partial counts and flags: never more than the labels
    assert ws(700, 440, 440) < 16 << 20
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1 << 11, 1 << 10, 1 << 10), (46341, 46341, 1)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, (1 << 31) - 1) > 0 and ws(2, 1, 1 << 30) == 0


# ------------------------------------------------------------------------------------------ the Python entries
def test_host_tensors_and_bad_arguments_are_refused(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a refusal reached the library")

    monkeypatch.setattr(metrics.H, "load", no_device)
    vol = torch.zeros((4, 5, 6))
    for call in (metrics.label_components, metrics.segment):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call(vol, 0.5)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call(vol.numpy(), 0.5)
    lab = torch.zeros((4, 5, 6), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.detection(lab, lab)
    with pytest.raises(ValueError, match="min_voxels"):
        metrics.segment(vol, 0.5, min_voxels=0)


# ------------------------------------------------------------------------------------------ the script
def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _no_device(mod, monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("the script went past its argument checks")

    monkeypatch.setattr(mod, "sr_create_model_and_diffusion", no_device)
    monkeypatch.setattr(mod.dist_util, "setup_dist", no_device)
    monkeypatch.setattr(mod._hip, "load", no_device)


def test_script_defaults_segment_nothing():
    mod = _script()
    args = mod.create_argparser().parse_args([])
    assert args.roi_threshold is None and args.roi_threshold_frac is None
    assert args.roi_connectivity == 26 and args.roi_min_voxels == 1
    assert not mod._segmenting(args) and mod._check_segmentation(None, args) is None


def _files(tmp_path):
    shape = (12, 16, 24)
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.ones(shape, dtype=np.float32))
    lab = np.zeros(shape, dtype=np.int32)
    lab[2:5, 3:6, 4:9] = 3
    np.save(tmp_path / "lab.npy", lab)
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]


CASES = {
    "both": (["--roi_threshold", "2.5", "--roi_threshold_frac", "0.4"], "--roi_threshold"),
    "with_labels": (["--roi_threshold", "2.5", "--roi_labels", "LAB"], "--roi_labels"),
    "frac_with_labels": (["--roi_threshold_frac", "0.4", "--roi_labels", "LAB"], "--roi_labels"),
    "with_background": (["--roi_threshold", "2.5", "--roi_background", "3"], "--roi_background"),
    "frac_with_background": (["--roi_threshold_frac", "0.4", "--roi_background", "3"], "--roi_background"),
    "no_target": (["--roi_threshold", "2.5"], "--target_samples"),
    "frac_no_target": (["--roi_threshold_frac", "0.4"], "--target_samples"),
    "frac_zero": (["--roi_threshold_frac", "0"], "--roi_threshold_frac"),
    "frac_one": (["--roi_threshold_frac", "1"], "--roi_threshold_frac"),
    "frac_negative": (["--roi_threshold_frac", "-0.2"], "--roi_threshold_frac"),
    "frac_nan": (["--roi_threshold_frac", "nan"], "--roi_threshold_frac"),
    "threshold_nan": (["--roi_threshold", "nan"], "--roi_threshold"),
    "connectivity_8": (["--roi_threshold", "2.5", "--roi_connectivity", "8"], "--roi_connectivity"),
    "connectivity_0": (["--roi_threshold", "2.5", "--roi_connectivity", "0"], "--roi_connectivity"),
    "min_voxels_0": (["--roi_threshold", "2.5", "--roi_min_voxels", "0"], "--roi_min_voxels"),
    "min_voxels_negative": (["--roi_threshold_frac", "0.4", "--roi_min_voxels", "-3"], "--roi_min_voxels"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_script_refuses_bad_segmentation_flags_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, names = CASES[case]
    argv = _files(tmp_path) + [str(tmp_path / "lab.npy") if a == "LAB" else a for a in extra]
    if "no_target" not in case:
        argv += ["--target_samples", str(tmp_path / "full.npz")]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    assert names in capsys.readouterr().err


@pytest.mark.parametrize("flags", [["--roi_threshold", "2.5"],
                                   ["--roi_threshold_frac", "0.4", "--roi_connectivity", "6", "--roi_min_voxels", "10"]],
                         ids=["absolute", "fraction"])
def test_script_accepts_good_flags_before_it_builds_the_model(flags, tmp_path, monkeypatch):
    """the same set-up with nothing wrong reaches the first device call: the refusals above are the checks' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path) + ["--target_samples", str(tmp_path / "full.npz")] + flags)
