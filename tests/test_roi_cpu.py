"""
CPU tier of the per-region statistics: the yardstick of tests/roi_ref.py is checked against
scipy.ndimage's labelled statistics so that it is not its own judge, roi_figures' arithmetic is checked on hand-made
records (draws, background, zero denominators), the two C entries are declared, exported and bound within ABI 13 and
refuse bad arguments on the host before any HIP call, load_labels and roi_index refuse what they cannot take, and
the inference script refuses a bad --roi_labels / --roi_background before a model is built.  No GPU is touched here.
"""

import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import roi_ref as R
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics, patches

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_roi_moments", "ddpm3d_roi_moments_workspace_bytes")
ONE_SHORT = "one byte less than the entry's own answer"


# ------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("scattered", [False, True], ids=["runs", "scattered"])
@pytest.mark.parametrize("offset", [0.0, 10.0])
def test_yardstick_agrees_with_scipy(scattered, offset):
    """|mean| <= 10 std, so sum x^2 / n - mean^2 has a condition number of at most 101: 101 times the summation bound,
    relative to the figure; extremes and counts are equal"""
    labels = R.labels_volume(scattered)
    xs, _ = R.volumes(offset)
    x = xs[2].astype(np.float64)                               # scipy on the same values in fp64
    found, lists = R.region_lists(labels)
    assert found == sorted(R.SIZES) and [len(a) for a in lists] == [R.SIZES[v] for v in found]
    recs = R.moments(xs[2], lists)
    for label, at, rec in zip(found, lists, recs):
        n, mean, std, mn, mx = R.stats(rec)
        tol = 101 * n * 2.0 ** -53
        want_mean, want_std = ndimage.mean(x, labels, label), ndimage.standard_deviation(x, labels, label)
        assert n == len(at) == int(ndimage.sum_labels(np.ones_like(x), labels, label))
        assert mn == ndimage.minimum(x, labels, label) and mx == ndimage.maximum(x, labels, label)
        assert abs(mean - want_mean) <= tol * np.abs(x.reshape(-1)[at]).mean(), (label, mean, want_mean)
        if n > 1:
            assert abs(mean) <= 10 * want_std                  # the premise of the factor
        assert abs(std - want_std) <= tol * want_std, (label, std, want_std)


def test_yardstick_errors_and_empty_regions():
    x = np.array([1.0, 2.0, 4.0, 8.0, -3.0], dtype=np.float32)
    y = np.array([1.5, 2.0, 3.0, -8.0, 0.0], dtype=np.float32)
    lists = [np.array([0, 2, 3]), np.array([], dtype=np.int64), np.array([4])]
    rec = R.moments(x, lists, y)
    assert rec[0] == [3.0, 13.0, 81.0, 1.0, 8.0, 16.5, 17.5, 0.25 + 1.0 + 256.0]
    assert rec[1] == [0.0, 0.0, 0.0, math.inf, -math.inf, 0.0, 0.0, 0.0]
    assert rec[2] == [1.0, -3.0, 9.0, -3.0, -3.0, -3.0, 3.0, 9.0]
    assert R.moments(x, lists)[0][R.SUM_E:] == [0.0, 0.0, 0.0]
    b = R.bound(x, lists, y)
    assert b[0][R.SUM_X] == 3 * 2.0 ** -53 * 13.0 and b[1] == [0.0] * R.REC and b[0][R.N] == 0.0


# ------------------------------------------------------------------------------------------ host figures
def _rec(values, target=None):
    v = np.asarray(values, dtype=np.float64)
    e = np.zeros_like(v) if target is None else v - np.asarray(target, dtype=np.float64)
    if v.size == 0:
        return [0.0, 0.0, 0.0, math.inf, -math.inf, 0.0, 0.0, 0.0]
    return [float(v.size), float(v.sum()), float((v * v).sum()), float(v.min()), float(v.max()), float(e.sum()),
            float(np.abs(e).sum()), float((e * e).sum())]


def test_roi_figures_on_hand_made_records():
    lesion_t, liver_t = [4.0, 6.0, 8.0, 6.0], [2.0, 2.0, 1.0, 3.0]
    lesion, liver = [3.0, 5.0, 7.0, 5.0], [2.0, 3.0, 1.0, 2.0]
    trec = [_rec(lesion_t), _rec(liver_t)]
    rec = [_rec(lesion, lesion_t), _rec(liver, liver_t)]
    f = metrics.roi_figures(rec, target_records=trec, labels=[3, 9], background=9)
    assert list(f) == [3, 9]
    a, g = f[3], f[9]
    assert (a["n"], a["mean"], a["min"], a["max"]) == (4, 5.0, 3.0, 7.0)
    assert a["std"] == pytest.approx(math.sqrt(2.0), rel=1e-15) and a["cov"] == pytest.approx(math.sqrt(2.0) / 5.0)
    assert a["mean_bias"] == -1.0 and a["mean_bias_rel"] == pytest.approx(-1.0 / 6.0)
    assert a["max_bias_rel"] == pytest.approx(-1.0 / 8.0) and a["rmse"] == 1.0 and a["mae"] == 1.0
    assert g["mean"] == 2.0 and g["std"] == pytest.approx(math.sqrt(0.5)) and g["mae"] == 0.5
    assert a["contrast"] == pytest.approx(5.0 / 2.0 - 1.0) and a["crc"] == pytest.approx(1.5 / 2.0)
    assert a["cnr"] == pytest.approx(3.0 / math.sqrt(0.5))
    assert not {"contrast", "crc", "cnr"} & set(g)              # the reference region has no contrast to itself
    assert not {"draw_means", "mean_std", "mean_z"} & set(a)
    plain = metrics.roi_figures(rec)
    assert list(plain) == [0, 1] and set(plain[0]) == {"n", "mean", "std", "min", "max", "cov"}
    assert set(metrics.roi_figures(rec, labels=[3, 9], background=9)[3]) == {"n", "mean", "std", "min", "max", "cov",
                                                                              "contrast", "cnr"}


def test_roi_figures_with_draws():
    target = [4.0, 6.0]
    draws = [[_rec([3.0, 5.0], target)], [_rec([5.0, 9.0], target)], [_rec([4.0, 6.0], target)]]
    f = metrics.roi_figures([_rec([4.0, 6.5], target)], target_records=[_rec(target)], labels=[12],
                            draw_records=draws)[12]
    assert f["draw_means"] == [4.0, 7.0, 5.0]
    want = float(np.std([4.0, 7.0, 5.0], ddof=1))
    assert f["mean_std"] == pytest.approx(want, rel=1e-15)
    assert f["mean_z"] == pytest.approx((16.0 / 3.0 - 5.0) / want, rel=1e-14)
    same = metrics.roi_figures([_rec([4.0, 6.0])], labels=[12], draw_records=draws[2:] * 2)[12]
    assert same["mean_std"] == 0.0 and same["mean_z"] is None     # no target: no z; and below a zero spread
    z = metrics.roi_figures([_rec(target, target)], target_records=[_rec(target)], draw_records=draws[2:] * 2)[0]
    assert z["mean_std"] == 0.0 and z["mean_z"] is None
    with pytest.raises(ValueError):
        metrics.roi_figures([_rec(target)], draw_records=draws[:1])


def test_roi_figures_zero_denominators_give_none():
    zero, empty, flat = _rec([1.0, -1.0], [0.0, 0.0]), _rec([]), _rec([2.0, 2.0], [0.0, 0.0])
    trec = [_rec([0.0, 0.0]), _rec([]), _rec([0.0, 0.0])]
    f = metrics.roi_figures([zero, empty, flat], target_records=trec, labels=[1, 2, 3], background=3)
    assert f[1]["mean"] == 0.0 and f[1]["cov"] is None and f[1]["mean_bias"] == 0.0
    assert f[1]["mean_bias_rel"] is None and f[1]["max_bias_rel"] is None and f[1]["rmse"] == 1.0
    assert f[1]["contrast"] == -1.0 and f[1]["crc"] is None     # the target's own contrast is 0 / 0
    assert f[1]["cnr"] is None                                  # the background is flat: std 0
    e = f[2]
    assert e["n"] == 0 and all(e[k] is None for k in ("mean", "std", "min", "max", "cov", "mean_bias", "mean_bias_rel",
                                                      "max_bias_rel", "rmse", "mae", "contrast", "crc", "cnr"))
    g = metrics.roi_figures([flat, zero], labels=[3, 1], background=1)
    assert g[3]["contrast"] is None and g[3]["cnr"] == pytest.approx(2.0)
    with pytest.raises(ValueError, match="background"):
        metrics.roi_figures([zero], labels=[1], background=4)
    with pytest.raises(ValueError):
        metrics.roi_figures([zero], labels=[1, 2])


def test_host_tensors_and_bad_labels_are_refused():
    lab = torch.zeros((4, 5, 6), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.roi_index(lab)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.roi_index(lab.numpy())


# ------------------------------------------------------------------------------------------ the C entries
def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    cols = dict((n, int(v)) for n, v in re.findall(r"\bDDPM3D_ROI_([A-Z0-9_]+) = (\d+)", hdr))
    mine = {k[4:]: getattr(_hip, k) for k in dir(_hip) if k.startswith("ROI_") and k[4:] in cols}
    assert cols == mine and cols["REC"] == 8 and sorted(cols.values()) == list(range(9))
    assert [getattr(R, k) for k in ("N", "SUM_X", "SUM_SQ_X", "MIN_X", "MAX_X", "SUM_E", "SUM_ABS_E", "SUM_SQ_E",
                                    "REC")] == [cols[k] for k in ("N", "SUM_X", "SUM_SQ_X", "MIN_X", "MAX_X", "SUM_E",
                                                                   "SUM_ABS_E", "SUM_SQ_E", "REC")]
    for name, value in (("MAX_REGIONS", _hip.ROI_MAX_REGIONS), ("CHUNK", _hip.ROI_CHUNK)):
        assert re.search(r"#define DDPM3D_ROI_%s %d\b" % (name, value), hdr) and value == 4096
    assert "roi.o" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert os.path.isfile(os.path.join(PKG, "csrc", "roi.hip"))


def _index(offsets=(0, 5, 5, 4101), entries=None, regions=None, **ptrs):
    """a descriptor with real host offsets and fake device pointers"""
    host = (ctypes.c_int64 * len(offsets))(*offsets) if offsets is not None else None
    p = dict(d_offsets=FAKE, d_chunks=FAKE, d_index=FAKE)
    p.update(ptrs)
    d = _hip.RoiIndex(len(offsets) - 1 if regions is None else regions, offsets[-1] if entries is None else entries,
                      host, p["d_offsets"], p["d_chunks"], p["d_index"])
    return d


def _moments(index="default", **over):
    lib = _hip.load()
    ix = _index() if index == "default" else index
    a = dict(est=FAKE, target=None, B=2, voxels=1 << 20, index=ix, ws=FAKE, ws_bytes=1 << 30, out=FAKE, stream=None)
    a.update(over)
    if a["ws_bytes"] == ONE_SHORT:
        a["ws_bytes"] = lib.ddpm3d_roi_moments_workspace_bytes(a["B"], a["index"]) - 1
        assert a["ws_bytes"] > 0
    rc = lib.ddpm3d_roi_moments(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


BIG = [0] + [1] * (_hip.ROI_MAX_REGIONS + 1)


@pytest.mark.parametrize("over", [
    dict(est=None), dict(out=None), dict(ws=None), dict(index=None),
    dict(B=0), dict(B=-2), dict(B=65), dict(voxels=0), dict(voxels=-1), dict(voxels=(1 << 40) + 1),
    dict(ws_bytes=0), dict(ws_bytes=ONE_SHORT), dict(ws=FAKE + 8),
], ids=lambda o: "-".join("%s=%s" % kv for kv in o.items())[:40])
def test_roi_moments_refuses_bad_arguments(over):
    rc, msg = _moments(**over)
    assert rc == _hip.E_INVAL and msg.startswith("roi_moments:"), (rc, msg)


@pytest.mark.parametrize("make", [
    lambda: _index(d_offsets=None), lambda: _index(d_chunks=None), lambda: _index(d_index=None),
    lambda: _hip.RoiIndex(1, 5, None, FAKE, FAKE, FAKE),                      # no host offsets
    lambda: _index(regions=0), lambda: _index(regions=-1), lambda: _index(BIG),
    lambda: _index(entries=-1), lambda: _index((0, (1 << 40) + 1)),
    lambda: _index((1, 5, 9)),                                                # does not start at 0
    lambda: _index((0, 7, 5, 9)),                                             # decreases
    lambda: _index((0, 5, 9), entries=10), lambda: _index((0, 5, 9), entries=8),   # ends elsewhere than entries
], ids=["d_offsets", "d_chunks", "d_index", "offsets", "R=0", "R<0", "R>max", "entries<0", "entries>2^40", "start",
        "decrease", "short", "long"])
def test_roi_moments_refuses_a_bad_index(make):
    ix = make()
    rc, msg = _moments(index=ix)
    assert rc == _hip.E_INVAL and msg.startswith("roi_moments:"), (rc, msg)
    assert _hip.load().ddpm3d_roi_moments_workspace_bytes(2, ix) == 0


def test_workspace_sizes():
    ws = _hip.load().ddpm3d_roi_moments_workspace_bytes
    rec = _hip.ROI_REC * 8
    assert ws(1, _index((0, 1))) == rec and ws(3, _index((0, 4096))) == 3 * rec
    assert ws(1, _index((0, 4097))) == 2 * rec
    assert ws(2, _index()) == 2 * (1 + 0 + 1) * rec                           # 5, 0 and 4096 entries
    assert ws(1, _index((0, 0, 0))) == rec                                    # nothing but empty regions: still a buffer
    assert ws(64, _index((0, 1 << 40))) == 64 * (1 << 28) * rec
    assert ws(1, _index([0] + [1] * _hip.ROI_MAX_REGIONS)) == rec
    for bad in (0, 65, -1):
        assert ws(bad, _index()) == 0
    assert ws(1, None) == 0


# ------------------------------------------------------------------------------------------ labels from files
def test_load_labels(tmp_path):
    lab = np.zeros((3, 4, 5), dtype=np.int16)
    lab[1, 2, 3], lab[0, 0, 0] = 7, 4000
    np.save(tmp_path / "a.npy", lab)
    np.savez(tmp_path / "b.npz", lab.astype(np.float32)[None])                # integral floats, a leading 1
    from guided_diffusion import tiff_io
    tiff_io.imwrite(str(tmp_path / "c.tif"), lab.astype(np.float32))
    for name in ("a.npy", "b.npz", "c.tif"):
        got = patches.load_labels(str(tmp_path / name))
        assert got.dtype == np.int32 and got.shape == (3, 4, 5) and np.array_equal(got, lab), name
    np.save(tmp_path / "half.npy", lab + 0.5)
    np.save(tmp_path / "neg.npy", -lab)
    np.save(tmp_path / "nan.npy", np.where(lab > 0, np.nan, 0.0))
    np.save(tmp_path / "huge.npy", lab.astype(np.int64) << 30)
    np.save(tmp_path / "flat.npy", lab[0])
    np.save(tmp_path / "bool.npy", lab > 0)
    for name in ("half", "neg", "nan", "huge", "flat", "bool"):
        with pytest.raises(ValueError):
            patches.load_labels(str(tmp_path / (name + ".npy")))
    assert patches.load_volume(str(tmp_path / "a.npy")).dtype == np.float32   # the volume loader is as it was


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


def test_script_defaults_run_no_region_statistics():
    mod = _script()
    args = mod.create_argparser().parse_args([])
    assert args.roi_labels == "" and args.roi_background == -1
    assert mod._load_roi(None, args, None) is None
    assert mod._write_metrics(args, "unused", None, None, None) is None


@pytest.mark.parametrize("case", ["no_target", "missing", "shape", "fraction", "negative", "none", "many",
                                  "background_absent", "background_zero"])
def test_script_refuses_bad_labels_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    shape = (12, 16, 24)                                                      # 4608 voxels: room for 4097 labels
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.zeros(shape, dtype=np.float32))
    lab = np.zeros(shape, dtype=np.int32)
    lab[2:5, 3:6, 4:9] = 3
    lab[6, 6, 6] = 8
    if case == "shape":
        lab = lab[:, :, :20]
    elif case == "fraction":
        lab = lab + 0.25
    elif case == "negative":
        lab[0, 0, 0] = -1
    elif case == "none":
        lab[:] = 0
    elif case == "many":
        lab = np.arange(lab.size, dtype=np.int32).reshape(shape)
        lab[lab > _hip.ROI_MAX_REGIONS + 1] = 0
    np.save(tmp_path / "lab.npy", lab)
    argv = ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path),
            "--roi_labels", str(tmp_path / ("nothing.npy" if case == "missing" else "lab.npy"))]
    if case != "no_target":
        argv += ["--target_samples", str(tmp_path / "full.npz")]
    if case.startswith("background"):
        argv += ["--roi_background", "5" if case == "background_absent" else "0"]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    assert ("--roi_background" if case.startswith("background") else "--roi_labels") in capsys.readouterr().err


def test_script_accepts_good_labels_before_it_builds_the_model(tmp_path, monkeypatch):
    """the same set-up with nothing wrong reaches the first device call: the refusals above are the checks' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    shape = (12, 16, 24)
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.zeros(shape, dtype=np.float32))
    lab = np.zeros(shape, dtype=np.int32)
    lab[2:5, 3:6, 4:9], lab[6, 6, 6] = 3, 8
    np.save(tmp_path / "lab.npy", lab)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path), "--target_samples",
                  str(tmp_path / "full.npz"), "--roi_labels", str(tmp_path / "lab.npy"), "--roi_background", "8"])
