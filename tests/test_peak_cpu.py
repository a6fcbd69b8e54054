"""
CPU tier of SUVpeak / MTV / TLG: metrics.sphere_footprint's run table against the brute-force
footprint of tests/peak_ref.py, its refusals, the C entry declared, exported and bound within ABI 13, every host
refusal of the entry (no HIP call is made: the pointers are fake), the Python entries' refusal of host tensors,
roi_figures' new figures against hand arithmetic, and the inference script's refusals of bad --voxel_spacing before
any device call.  No GPU is touched here.
"""

import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import peak_ref as P
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first

# spacing (mm) -> (radii, taps) of the 1 cm^3 sphere; no lattice point lies within 3e-3 mm of any of these spheres
FOOTPRINTS = {
    (2.0, 2.0, 2.0): ((3, 3, 3), 123),
    (2.0, 2.0, 3.0): ((3, 3, 2), 73),
    (3.27, 2.0, 1.5): ((1, 3, 4), 105),
    (6.0, 2.0, 0.775): ((1, 3, 8), 93),
    (4.0, 4.0, 4.0): ((1, 1, 1), 19),
    (7.0, 7.0, 7.0): ((0, 0, 0), 1),
}


# ------------------------------------------------------------------------------------------ the footprint
def test_radius_of_one_cubic_centimetre():
    assert abs(P.radius_mm() - 6.2035) < 5e-5
    assert metrics.sphere_footprint((2, 2, 2)).radius_mm == pytest.approx(P.radius_mm(), rel=1e-15)


@pytest.mark.parametrize("spacing", sorted(FOOTPRINTS), ids=str)
def test_run_table_expands_to_the_brute_force_footprint(spacing):
    radii, taps = FOOTPRINTS[spacing]
    assert P.margin_mm(spacing) > 3e-3                       # not an edge case: no voxel centre sits on the sphere
    want, want_radii = P.trimmed(P.footprint(spacing))
    assert want_radii == radii and int(want.sum()) == taps
    fp = metrics.sphere_footprint(spacing)
    assert fp.radii == radii and fp.taps == taps and fp.spacing == spacing and fp.volume_mm3 == 1000.0
    assert len(fp.half_w) == 2 * radii[0] + 1 and all(len(row) == 2 * radii[1] + 1 for row in fp.half_w)
    assert np.array_equal(P.expand(fp.radii, fp.half_w), want)
    assert list(fp.table) == [w for row in fp.half_w for w in row]
    assert fp.half_w[radii[0]][radii[1]] == radii[2]


def test_another_volume_and_integer_spacing():
    fp = metrics.sphere_footprint([2, 2, 2], volume_mm3=4000)
    want, radii = P.trimmed(P.footprint((2.0, 2.0, 2.0), 4000.0))
    assert fp.radii == radii and np.array_equal(P.expand(fp.radii, fp.half_w), want) and fp.volume_mm3 == 4000.0


@pytest.mark.parametrize("spacing", [(0.6, 2.0, 2.0), (2.0, 0.6, 2.0), (2.0, 2.0, 0.6), (0.0, 2.0, 2.0),
                                     (2.0, -2.0, 2.0), (2.0, 2.0, float("nan")), (float("inf"), 2.0, 2.0),
                                     (2.0, 2.0), (2.0, 2.0, 2.0, 2.0), 2.0, None, ("a", 2.0, 2.0)], ids=str)
def test_footprint_refuses_bad_spacings(spacing):
    with pytest.raises(ValueError, match="sphere_footprint:"):
        metrics.sphere_footprint(spacing)


def test_footprint_names_the_radius_limit_and_allows_the_largest():
    with pytest.raises(ValueError, match="DDPM3D_PEAK_MAX_RADIUS = 8"):
        metrics.sphere_footprint((0.6, 0.6, 0.6))
    assert metrics.sphere_footprint((0.69, 0.69, 0.69)).radii == (8, 8, 8)
    assert P.radius_mm() / 0.6 > 9 > P.radius_mm() / 0.69 > 8


def test_footprint_takes_any_real_number_for_the_volume():
    want = metrics.sphere_footprint((2.0, 2.0, 2.0), 4000.0)
    for volume in (4000, np.float32(4000.0), np.array(4000.0), np.int64(4000)):
        fp = metrics.sphere_footprint((2.0, 2.0, 2.0), volume)
        assert fp.half_w == want.half_w and fp.volume_mm3 == 4000.0 and type(fp.volume_mm3) is float


@pytest.mark.parametrize("volume", [0, 0.0, -1000.0, float("nan"), float("inf"), None, "1000", True, [1000.0, 2.0]],
                         ids=str)
def test_footprint_refuses_bad_volumes(volume):
    with pytest.raises(ValueError, match="sphere_footprint: the volume"):
        metrics.sphere_footprint((2.0, 2.0, 2.0), volume)


# ------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_on_a_case_worked_by_hand():
    fp = P.footprint((4.0, 4.0, 4.0))                        # the centre, its 6 face and 12 edge neighbours
    assert int(fp.sum()) == 19
    x = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    mean, n, bound = P.sphere_mean(x, fp)
    assert n[1, 1, 1] == 19 and mean[1, 1, 1] == pytest.approx((x.sum() - x[::2, ::2, ::2].sum()) / 19)
    assert n[0, 0, 0] == 7 and mean[0, 0, 0] == pytest.approx((0 + 1 + 3 + 9 + 4 + 10 + 12) / 7)
    assert bound[0, 0, 0] == pytest.approx(9 * 2.0 ** -24 * 39 / 7)
    keep = np.ones((3, 3, 3), dtype=np.uint8)
    keep[0, 0, 1] = keep[0, 0, 0] = 0
    mean, n, _ = P.sphere_mean(x, fp, keep)
    assert n[0, 0, 0] == 5 and mean[0, 0, 0] == pytest.approx((3 + 9 + 4 + 10 + 12) / 5)   # keep does not blank v
    mean, n, bound = P.sphere_mean(x, fp, np.zeros((3, 3, 3), dtype=np.uint8))
    assert not n.any() and not mean.any() and not bound.any()


# ------------------------------------------------------------------------------------------ the C entry
def test_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert "ddpm3d_sphere_mean" in declared and "ddpm3d_sphere_mean" in _hip.EXPORTS
    assert hasattr(lib, "ddpm3d_sphere_mean")
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    assert int(re.search(r"#define DDPM3D_PEAK_MAX_RADIUS (\d+)\b", hdr).group(1)) == _hip.PEAK_MAX_RADIUS == 8
    assert "PERCIST" in hdr
    assert re.search(r"^OBJS\s*:=.*\bpeak\.o\b", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M)
    assert os.path.isfile(os.path.join(PKG, "csrc", "peak.hip"))


def _table(spacing=(2.0, 2.0, 2.0)):
    fp = metrics.sphere_footprint(spacing)
    return fp.radii[0], fp.radii[1], [list(row) for row in fp.half_w]


def _call(table=None, **over):
    lib = _hip.load()
    r0, r1, rows = _table()
    a = dict(vol=FAKE, keep=None, B=1, D=20, H=30, W=40, r0=r0, r1=r1, half_w=rows if table is None else table,
             out=2 * FAKE, stream=None)
    a.update(over)
    if a["half_w"] is not None:
        flat = [w for row in a["half_w"] for w in row]
        a["half_w"] = (ctypes.c_int32 * len(flat))(*flat)
    rc = lib.ddpm3d_sphere_mean(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


def _edited(i, j, w, mirror=False):
    rows = _table()[2]
    rows[i][j] = w
    if mirror:                                              # keep the table symmetric: the other check must speak
        rows[len(rows) - 1 - i][j] = rows[i][len(rows[0]) - 1 - j] = w
        rows[len(rows) - 1 - i][len(rows[0]) - 1 - j] = w
    return rows


BAD = {
    "vol_null": dict(vol=None), "out_null": dict(out=None), "half_w_null": dict(half_w=None),
    "in_place": dict(out=FAKE),
    "B_0": dict(B=0), "B_negative": dict(B=-1), "B_above_max": dict(B=_hip.MAX_DRAWS + 1),
    "D_0": dict(D=0), "H_0": dict(H=0), "W_0": dict(W=0), "W_negative": dict(W=-64),
    "voxels_2_31": dict(D=1 << 11, H=1 << 10, W=1 << 10), "plane_2_32": dict(D=1 << 16, H=1 << 16, W=1),
    "voxels_just_above": dict(D=46341, H=46341, W=1),
    "r0_negative": dict(r0=-1), "r0_9": dict(r0=9), "r1_negative": dict(r1=-1), "r1_9": dict(r1=9),
    "entry_9": dict(table=_edited(3, 3, 9)), "entry_minus_2": dict(table=_edited(0, 0, -2, mirror=True)),
    "entry_9_mirrored": dict(table=_edited(1, 1, 9, mirror=True)),
    "centre_absent": dict(table=_edited(3, 3, -1)),
    "not_symmetric_in_dz": dict(table=_edited(0, 3, 2)), "not_symmetric_in_dy": dict(table=_edited(3, 0, 2)),
    "not_symmetric_absent": dict(table=_edited(1, 1, -1)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_sphere_mean_refuses_bad_arguments(case):
    rc, msg = _call(**BAD[case])
    assert rc == _hip.E_INVAL and msg.startswith("sphere_mean:"), (rc, msg)


def test_refusals_name_what_is_wrong():
    assert "null" in _call(vol=None)[1] and "out must not be vol" in _call(out=FAKE)[1]
    assert "B=65" in _call(B=65)[1] and "2^31 - 1" in _call(D=46341, H=46341, W=1)[1]
    assert "r0=9" in _call(r0=9)[1] and "half_w[3][3]=9" in _call(table=_edited(3, 3, 9))[1]
    assert "centre row" in _call(table=_edited(3, 3, -1))[1] and "symmetric" in _call(table=_edited(0, 3, 2))[1]


# ------------------------------------------------------------------------------------------ the Python entries
def test_host_tensors_and_bad_arguments_are_refused(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a refusal reached the library")

    monkeypatch.setattr(metrics.H, "load", no_device)
    fp = metrics.sphere_footprint((2.0, 2.0, 2.0))
    vol = torch.zeros((4, 5, 6))
    for bad in (vol, vol.numpy(), vol.double()):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            metrics.sphere_mean(bad, fp)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            metrics.roi_peak(bad, None, fp)


# ------------------------------------------------------------------------------------------ roi_figures
#          N    SUM_X  SUM_SQ_X  MIN  MAX   SUM_E  SUM_ABS_E  SUM_SQ_E
EST = [[4.0,  10.0,   30.0,    1.0, 4.0,  2.0,   2.0,       1.5],
       [2.0,   3.0,    5.0,    1.0, 2.0, -1.0,   1.0,       0.5],
       [0.0,   0.0,    0.0,    math.inf, -math.inf, 0.0, 0.0, 0.0]]
TGT = [[4.0,   8.0,   20.0,    1.0, 3.0,  0.0,   0.0,       0.0],
       [2.0,   4.0,    8.0,    2.0, 2.0,  0.0,   0.0,       0.0],
       [0.0,   0.0,    0.0,    math.inf, -math.inf, 0.0, 0.0, 0.0]]
DRAWS = [EST, TGT, EST]
NEW = {"volume_ml", "tlg", "tlg_bias_rel", "peak", "peak_bias_rel", "draw_peaks", "peak_std"}


def test_roi_figures_with_spacing_equals_hand_arithmetic():
    f = metrics.roi_figures(EST, target_records=TGT, labels=[3, 5, 9], spacing=(2.0, 2.5, 4.0))
    assert f[3]["volume_ml"] == pytest.approx(4 * 20.0 / 1000) and f[3]["tlg"] == pytest.approx(0.08 * 2.5)
    assert f[3]["tlg_bias_rel"] == pytest.approx((0.2 - 0.16) / 0.16)
    assert f[5]["volume_ml"] == pytest.approx(0.04) and f[5]["tlg"] == pytest.approx(0.06)
    assert f[5]["tlg_bias_rel"] == pytest.approx(-0.25)
    assert f[9]["volume_ml"] == 0.0 and f[9]["tlg"] is None and f[9]["tlg_bias_rel"] is None
    assert not {"peak", "peak_bias_rel", "draw_peaks", "peak_std"} & set(f[3])
    t = metrics.roi_figures(TGT, labels=[3, 5, 9], spacing=(2.0, 2.5, 4.0))
    assert t[3]["tlg"] == pytest.approx(0.16) and "tlg_bias_rel" not in t[3]


def test_roi_figures_with_peaks_equals_hand_arithmetic():
    f = metrics.roi_figures(EST, target_records=TGT, draw_records=DRAWS, spacing=(1.0, 1.0, 1.0),
                            peaks=[3.0, 1.5, -math.inf], target_peaks=[2.0, 0.0, -math.inf],
                            draw_peaks=[[3.0, 1.0, -math.inf], [2.0, 2.0, -math.inf], [4.0, 3.0, -math.inf]])
    assert f[0]["peak"] == 3.0 and f[0]["peak_bias_rel"] == pytest.approx(0.5)
    assert f[0]["draw_peaks"] == [3.0, 2.0, 4.0] and f[0]["peak_std"] == pytest.approx(1.0)
    assert f[1]["peak"] == 1.5 and f[1]["peak_bias_rel"] is None            # a zero denominator
    assert f[1]["peak_std"] == pytest.approx(1.0)
    assert f[2]["peak"] is None and f[2]["peak_bias_rel"] is None and f[2]["peak_std"] is None
    assert f[2]["draw_peaks"] == [None, None, None]
    assert NEW <= set(f[0])


def test_roi_figures_without_the_new_arguments_is_unchanged():
    old = metrics.roi_figures(EST, target_records=TGT, labels=[3, 5, 9], background=5, draw_records=DRAWS)
    new = metrics.roi_figures(EST, target_records=TGT, labels=[3, 5, 9], background=5, draw_records=DRAWS,
                              spacing=(2.0, 2.0, 2.0), peaks=[1.0, 1.0, 1.0], target_peaks=[1.0, 1.0, 1.0],
                              draw_peaks=[[1.0] * 3] * 3)
    for label in (3, 5, 9):
        assert not NEW & set(old[label])
        assert {k: v for k, v in new[label].items() if k not in NEW} == old[label]
        assert list(new[label])[:len(old[label])] == list(old[label])      # the new figures come after the old
    assert list(old[3]) == ["n", "mean", "std", "min", "max", "cov", "mean_bias", "mean_bias_rel", "max_bias_rel",
                            "rmse", "mae", "contrast", "crc", "cnr", "draw_means", "mean_std", "mean_z"]
    assert old[3]["mean"] == 2.5 and old[3]["mean_bias_rel"] == pytest.approx(0.25) and old[3]["max"] == 4.0


def test_roi_figures_refuses_bad_new_arguments():
    with pytest.raises(ValueError, match="voxel spacing"):
        metrics.roi_figures(EST, spacing=(2.0, 2.0))
    with pytest.raises(ValueError, match="voxel spacing"):
        metrics.roi_figures(EST, spacing=(2.0, 0.0, 2.0))
    with pytest.raises(ValueError, match="peaks"):
        metrics.roi_figures(EST, peaks=[1.0])
    with pytest.raises(ValueError, match="draw_peaks"):
        metrics.roi_figures(EST, draw_peaks=[[1.0] * 3])
    with pytest.raises(ValueError, match="need a spacing"):
        metrics.roi_report(None, None, None, labels=[1], volume_mm3=500.0)
    with pytest.raises(ValueError, match="need a spacing"):
        metrics.roi_report(None, None, None, labels=[1], target_peaks=[1.0])
    fp = metrics.sphere_footprint((2.0, 2.0, 2.0))
    with pytest.raises(ValueError, match="must be of the spacing"):
        metrics.roi_report(None, None, None, labels=[1], spacing=(2.0, 2.0, 3.0), footprint=fp)
    with pytest.raises(ValueError, match="its own volume_mm3"):
        metrics.roi_report(None, None, None, labels=[1], spacing=(2.0, 2.0, 2.0), footprint=fp, volume_mm3=1000.0)


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


def _files(tmp_path):
    shape = (12, 16, 24)
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.ones(shape, dtype=np.float32))
    lab = np.zeros(shape, dtype=np.int32)
    lab[2:5, 3:6, 4:9] = 3
    np.save(tmp_path / "lab.npy", lab)
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]


def test_script_default_is_no_spacing():
    mod = _script()
    args = mod.create_argparser().parse_args([])
    assert args.voxel_spacing is None and mod._check_spacing(None, args) is None


REGIONS = ["--roi_labels", "LAB"]
CASES = {
    "no_regions": (["--voxel_spacing", "2", "2", "2"], "needs regions"),
    "no_target": (["--voxel_spacing", "2", "2", "2"] + REGIONS, "--target_samples"),
    "two_numbers": (["--voxel_spacing", "2", "2"] + REGIONS, "three numbers"),
    "four_numbers": (["--voxel_spacing", "2", "2", "2", "2"] + REGIONS, "three numbers"),
    "no_number": (["--voxel_spacing"] + REGIONS, "--voxel_spacing"),
    "not_a_number": (["--voxel_spacing", "2", "two", "2"] + REGIONS, "--voxel_spacing"),
    "zero": (["--voxel_spacing", "2", "0", "2"] + REGIONS, "positive finite"),
    "negative": (["--voxel_spacing", "-2", "2", "2"] + REGIONS, "positive finite"),
    "nan": (["--voxel_spacing", "2", "2", "nan"] + REGIONS, "positive finite"),
    "inf": (["--voxel_spacing", "inf", "2", "2"] + REGIONS, "positive finite"),
    "too_fine": (["--voxel_spacing", "2", "0.6", "2"] + REGIONS, "DDPM3D_PEAK_MAX_RADIUS"),
    "too_fine_threshold": (["--voxel_spacing", "0.5", "2", "2", "--roi_threshold", "0.5"], "DDPM3D_PEAK_MAX_RADIUS"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_script_refuses_bad_voxel_spacing_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, names = CASES[case]
    argv = _files(tmp_path) + [str(tmp_path / "lab.npy") if a == "LAB" else a for a in extra]
    if case != "no_target":
        argv += ["--target_samples", str(tmp_path / "full.npz")]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert names in err and "--voxel_spacing" in err


@pytest.mark.parametrize("flags", [["--roi_labels", "LAB"], ["--roi_threshold", "0.5"],
                                   ["--roi_threshold_frac", "0.4", "--num_draws", "2"]],
                         ids=["labels", "absolute", "fraction-draws"])
def test_script_accepts_a_good_spacing_before_it_builds_the_model(flags, tmp_path, monkeypatch):
    """the same set-up with nothing wrong reaches the first device call: the refusals above are the checks' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    flags = [str(tmp_path / "lab.npy") if a == "LAB" else a for a in flags]
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path) + ["--target_samples", str(tmp_path / "full.npz"), "--voxel_spacing", "3.27", "2",
                                     "1.5"] + flags)


def test_script_permutes_the_spacing_with_the_volumes():
    mod = _script()
    parser = mod.create_argparser()
    args = parser.parse_args(["--voxel_spacing", "3.27", "2.0", "1.5", "--target_samples", "t.npz", "--roi_labels",
                              "l.npz"])
    peak = mod._check_spacing(parser, args)
    assert peak["spacing"] == (2.0, 1.5, 3.27)                # (D, H, W) of the file -> (H, W, Z) of the volumes
    assert peak["footprint"].radii == (3, 4, 1) and peak["footprint"].taps == 105
