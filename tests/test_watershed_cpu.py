"""
CPU tier of the watershed split: the yardstick of tests/watershed_ref.py on hand-worked cases,
metrics.merge_basins against it on random graphs (ties in saddle and height included), the four C entries declared,
exported and bound within ABI 13, every host refusal of both entries (no HIP call is made: the pointers are fake),
the Python entries' argument checks and the inference script's refusals of bad --roi_split_prominence /
--roi_split_fwhm before any device call.  No GPU is touched here.
"""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import watershed_ref as R
from conftest import PKG, ROOT
from guided_diffusion import _hip, metrics

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first
ENTRIES = ("ddpm3d_basins", "ddpm3d_basins_workspace_bytes", "ddpm3d_basin_saddles",
           "ddpm3d_basin_saddles_workspace_bytes")
INF = float("inf")


def row(values, labels=None):
    h = np.array(values, dtype=np.float32).reshape(1, 1, -1)
    lab = np.ones(h.shape, dtype=np.int32) if labels is None else np.array(labels, dtype=np.int32).reshape(h.shape)
    return h, lab


# ------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_row_with_two_peaks_and_a_known_saddle():
    h, lab = row([3, 1, 2, 5, 4])
    for c in (6, 18, 26):
        peaks, n, longest = R.basins(h, lab, c)
        assert peaks.reshape(-1).tolist() == [0, 0, 3, 3, 3] and n == 2 and longest == 1
        pairs, saddle = R.saddles(h, lab, peaks, c)
        assert pairs.tolist() == [[0, 3]] and saddle.tolist() == [1.0]       # min(1, 2) across the border 1 | 2
    # the lesser peak (3) stands 2 above the saddle (1): merged iff not 2 >= P
    assert [R.split(lab, h, P)[1] for P in (0.0, 1.0, 2.0, 2.5, INF)] == [2, 2, 2, 1, 1]
    out, n, info = R.split(lab, h, 1.0)
    assert out.reshape(-1).tolist() == [1, 1, 2, 2, 2] and info["parent"] == [1, 1]
    assert info == {"n_before": 1, "n_basins": 2, "n_edges": 1, "n_after": 2, "parent": [1, 1]}


def test_yardstick_tie_break_on_a_constant_row():
    h, lab = row([7, 7, 7, 7, 7, 7])
    peaks, n, longest = R.basins(h, lab, 6)
    assert peaks.reshape(-1).tolist() == [0] * 6 and n == 1 and longest == 5     # each voxel's parent is its left one
    h, lab = row([1, 2, 2, 1])
    assert R.basins(h, lab, 6)[0].reshape(-1).tolist() == [1, 1, 1, 1]           # of the two 2s the lower index wins


def test_yardstick_labels_nan_and_infinities():
    h, lab = row([1, 2, 3, 4], labels=[1, 1, 2, 2])
    assert R.basins(h, lab, 26)[0].reshape(-1).tolist() == [1, 1, 3, 3]          # 2 | 3 touch but do not connect
    assert R.saddles(h, lab, R.basins(h, lab, 26)[0], 26)[0].shape == (0, 2)
    h, lab = row([1, np.nan, 3, 0], labels=[1, 1, 1, 0])
    assert R.basins(h, lab, 26)[0].reshape(-1).tolist() == [0, -1, 2, -1]        # NaN is background and separates
    h, lab = row([-INF, -INF, 0, INF, INF])
    # voxel 0 has no neighbour of greater key (its equal has the larger index): a peak at -inf; 4 climbs to 3
    assert R.basins(h, lab, 26)[0].reshape(-1).tolist() == [0, 3, 3, 3, 3]


def test_yardstick_prominence_zero_and_infinity():
    h, lab = R.two_blobs(noise=0.1)
    _, n_basins, _ = R.basins(h, lab, 6)
    out0, n0, _ = R.split(lab, h, 0.0, 6)
    assert n0 == n_basins > 2                                                # P = 0 unites nothing
    out, n, info = R.split(lab, h, INF, 6)
    assert n == 1 and np.array_equal(out, lab) and info["parent"] == [1]     # P = inf gives back the components


def test_yardstick_inf_minus_inf_unites():
    h, lab = row([INF, 0, INF])
    peaks, n, _ = R.basins(h, lab, 6)
    assert peaks.reshape(-1).tolist() == [0, 0, 2] and n == 2
    assert R.split(lab, h, 1e30)[1] == 2                                     # inf - 0 >= P: the peak stands
    h, lab = row([INF, INF, 0, INF])                                         # saddle min(inf, 0) = 0 again
    assert R.split(lab, h, 1e30)[1] == 2
    h, lab = row([INF, 1, INF], labels=[1, 1, 1])
    h[0, 0, 1] = INF                                                         # one plateau of inf: one basin
    assert R.basins(h, lab, 6)[1] == 1
    # two inf peaks whose saddle is inf: a U of inf around a finite voxel, the arms split by the index tie-break
    h = np.array([[[INF, 0, INF], [INF, INF, INF]]], dtype=np.float32).reshape(1, 2, 3)
    lab = np.ones(h.shape, dtype=np.int32)
    peaks, n, _ = R.basins(h, lab, 6)
    assert n == 2 and R.saddles(h, lab, peaks, 6)[1].tolist() == [INF]
    assert R.split(lab, h, 1e30, 6)[1] == 1 and R.split(lab, h, INF, 6)[1] == 1     # inf - inf is NaN: unites
    assert R.split(lab, h, 0.0, 6)[1] == 1                                   # and so it does at P = 0: NaN >= 0 fails


def test_yardstick_plateau_and_pieces_coarsen():
    h, lab = R.u_plateau()
    _, n, _ = R.basins(h, lab, 26)
    assert n > 1 and R.split(lab, h, 1e-9)[1] == 1
    h, lab = R.two_blobs()
    out, n, _ = R.split(lab, h, 0.05)
    assert n == 2 and np.bincount(out.reshape(-1))[1:].tolist() == [779, 545]
    h, lab = R.two_blobs(noise=0.1)
    for c in (6, 26):
        counts = [R.split(lab, h, P, c)[1] for P in (0.0, 0.05, 0.1, 0.2, 0.3, 0.5, INF)]
        assert counts == sorted(counts, reverse=True) and counts[-1] == 1, counts


def test_print_the_two_blob_table():
    """the README's table: pieces of the 12 x 20 x 28 two-blob volume against the prominence"""
    P = (0.05, 0.1, 0.2, 0.3, 0.5)
    print("\nconnectivity  noise  basins  " + "  ".join("P=%g" % p for p in P))
    for noise in (0.0, 0.1):
        h, lab = R.two_blobs(noise=noise)
        for c in (6, 26):
            print("%12d  %5g  %6d  " % (c, noise, R.basins(h, lab, c)[1])
                  + "  ".join("%*d" % (len("P=%g" % p), R.split(lab, h, p, c)[1]) for p in P))


# ------------------------------------------------------------------------------------------ merge_basins
def _expected_pieces(index, height, pairs, saddle, P):
    full = np.zeros(int(index.max()) + 1, dtype=np.float32)
    full[index] = height
    cluster = R.merge(full, pairs, saddle, P)
    return R.number(np.array([cluster.get(int(p), int(p)) for p in index]))


@pytest.mark.parametrize("levels", [None, 4], ids=["distinct", "ties"])
@pytest.mark.parametrize("seed", range(6))
def test_merge_basins_against_the_yardstick(seed, levels):
    index, height, pairs, saddle = R.random_graph(60, 150, seed, levels)
    for P in (0.0, 0.1, 0.3, 0.5, 1.0, 2.0, INF):
        want, n_want = _expected_pieces(index, height, pairs, saddle, P)
        got, n = metrics.merge_basins(index, height, pairs, saddle, P)
        assert n == n_want and np.array_equal(got, want), (seed, levels, P)
    assert metrics.merge_basins(index, height, pairs, saddle, 0.0)[1] >= metrics.merge_basins(
        index, height, pairs, saddle, 0.5)[1]


def test_merge_basins_hand_cases_and_numbering():
    index = np.array([4, 9, 20])
    height = np.array([5.0, 3.0, 4.0], dtype=np.float32)
    pairs = np.array([[4, 9], [9, 20]])
    saddle = np.array([1.0, 2.5], dtype=np.float32)
    # edge (9, 20) first (saddle 2.5): lesser peak 9 stands 0.5 above it; then (4, .) at saddle 1
    assert metrics.merge_basins(index, height, pairs, saddle, 0.4)[0].tolist() == [1, 2, 3]
    assert metrics.merge_basins(index, height, pairs, saddle, 0.5)[0].tolist() == [1, 2, 3]
    assert metrics.merge_basins(index, height, pairs, saddle, 0.6)[0].tolist() == [1, 2, 2]     # 9 joins 20: peak 4.0
    assert metrics.merge_basins(index, height, pairs, saddle, 3.0)[0].tolist() == [1, 2, 2]     # 4.0 - 1 >= 3 stands
    got, n = metrics.merge_basins(index, height, pairs, saddle, 3.5)
    assert got.tolist() == [1, 1, 1] and n == 1
    # numbering follows the pieces' first voxels, not their peaks
    got, n = metrics.merge_basins(index, height, pairs, saddle, 0.6, first_voxel=[7, 2, 3])
    assert got.tolist() == [2, 1, 1] and n == 2
    assert metrics.merge_basins([], [], np.zeros((0, 2)), [], 1.0)[1] == 0
    for bad in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="prominence"):
            metrics.merge_basins(index, height, pairs, saddle, bad)
    with pytest.raises(ValueError, match="no peak"):
        metrics.merge_basins(index, height, np.array([[4, 10]]), saddle[:1], 1.0)


# ------------------------------------------------------------------------------------------ the C entries
def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.ABI_VERSION == 13
    assert _hip.load().ddpm3d_abi_version() == 13
    assert "watershed.o" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert os.path.isfile(os.path.join(PKG, "csrc", "watershed.hip"))


def _basins(**over):
    lib = _hip.load()
    a = dict(height=FAKE, labels=FAKE + (1 << 24), connectivity=26, D=20, H=30, W=40, peaks=FAKE + (2 << 24), ws=FAKE,
             ws_bytes=1 << 20, status=FAKE, stream=None)
    a.update(over)
    rc = lib.ddpm3d_basins(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


def _saddles(**over):
    lib = _hip.load()
    a = dict(height=FAKE, labels=FAKE, peaks=FAKE, connectivity=26, D=20, H=30, W=40, cap=100, pairs=FAKE,
             saddle=FAKE, ws=FAKE, ws_bytes=1 << 20, status=FAKE, stream=None)
    a.update(over)
    rc = lib.ddpm3d_basin_saddles(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


SHAPES = [dict(D=0), dict(H=0), dict(W=0), dict(D=-1), dict(W=-64), dict(D=1 << 11, H=1 << 10, W=1 << 10),
          dict(D=1, H=1 << 16, W=1 << 16), dict(D=46341, H=46341, W=1)]
COMMON = [dict(connectivity=0), dict(connectivity=4), dict(connectivity=8), dict(connectivity=27),
          dict(connectivity=-6)] + SHAPES + [dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=15), dict(ws=FAKE + 8),
                                             dict(ws=FAKE + 4)]
IDS = lambda o: "-".join("%s=%s" % kv for kv in o.items())[:40]


@pytest.mark.parametrize("over", [dict(height=None), dict(labels=None), dict(peaks=None), dict(status=None)] + COMMON
                         + [dict(peaks=FAKE), dict(peaks=FAKE + (1 << 24) + 4), dict(peaks=FAKE + 20 * 30 * 40 * 4 - 4)],
                         ids=IDS)
def test_basins_refuses_bad_arguments(over):
    rc, msg = _basins(**over)
    assert rc == _hip.E_INVAL and msg.startswith("basins:"), (rc, msg)


@pytest.mark.parametrize("over", [dict(height=None), dict(labels=None), dict(peaks=None), dict(status=None),
                                  dict(pairs=None), dict(saddle=None), dict(cap=-1), dict(cap=-(1 << 31))] + COMMON,
                         ids=IDS)
def test_basin_saddles_refuses_bad_arguments(over):
    rc, msg = _saddles(**over)
    assert rc == _hip.E_INVAL and msg.startswith("basin_saddles:"), (rc, msg)


def test_workspace_sizes():
    lib = _hip.load()
    for ws in (lib.ddpm3d_basins_workspace_bytes, lib.ddpm3d_basin_saddles_workspace_bytes):
        for shape in ((1, 1, 1), (20, 30, 40), (700, 440, 440), (1, 1, (1 << 31) - 1), ((1 << 31) - 1, 1, 1)):
            assert ws(*shape) == 16, shape
        for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1 << 11, 1 << 10, 1 << 10), (46341, 46341, 1)):
            assert ws(*bad) == 0, bad


# ------------------------------------------------------------------------------------------ the Python entries
class _OnDevice(torch.Tensor):
    """a host tensor that says it lives on the device: the argument checks past `is_cuda` can be reached without one"""
    is_cuda = True


def _pretend(t):
    return t.as_subclass(_OnDevice)


def test_python_entries_refuse_bad_arguments_before_any_launch(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a refusal reached the library")

    monkeypatch.setattr(metrics.H, "load", no_device)
    h = torch.zeros((4, 5, 6))
    lab = torch.zeros((4, 5, 6), dtype=torch.int32)
    for call in (lambda a, b: metrics.basins(a, b), lambda a, b: metrics.basin_saddles(a, b, b),
                 lambda a, b: metrics.split_components(b, a, 1.0)):
        with pytest.raises(ValueError, match="must live on the GPU"):
            call(h, lab)
        with pytest.raises(ValueError, match="must live on the GPU"):
            call(h.numpy(), lab.numpy())
        with pytest.raises(ValueError, match="must live on the GPU"):
            call(_pretend(h), lab)
    dh, dl = _pretend(h), _pretend(lab)
    with pytest.raises(AssertionError, match="reached the library"):
        metrics.basins(dh, dl)                                # the pretended tensors pass every check
    for bad_h, bad_l, what in ((_pretend(h.double()), dl, "height"), (_pretend(torch.zeros((5, 6))), dl, "height"),
                               (_pretend(torch.zeros((4, 5, 6, 1))[..., 0].transpose(0, 1)), dl, "height"),
                               (dh, _pretend(lab.long()), "labels"), (dh, _pretend(lab.float()), "labels"),
                               (dh, _pretend(torch.zeros((4, 5, 7), dtype=torch.int32)), "labels"),
                               (_pretend(torch.zeros((0, 5, 6))), _pretend(torch.zeros((0, 5, 6), dtype=torch.int32)),
                                "voxels")):
        for call in (lambda a, b: metrics.basins(a, b), lambda a, b: metrics.split_components(b, a, 1.0)):
            with pytest.raises(ValueError, match=what):
                call(bad_h, bad_l)
    with pytest.raises(ValueError, match="peaks"):
        metrics.basin_saddles(dh, dl, _pretend(lab.long()))
    for c in (0, 8, 27, "26"):
        with pytest.raises(ValueError, match="connectivity"):
            metrics.basins(dh, dl, connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            metrics.split_components(dl, dh, 1.0, connectivity=c)
    for p in (float("nan"), -1.0, -INF):
        with pytest.raises(ValueError, match="prominence"):
            metrics.split_components(dl, dh, p)
    for m in (0, -3, 2.5):
        with pytest.raises(ValueError, match="max_basins"):
            metrics.split_components(dl, dh, 1.0, max_basins=m)
    for cap in (-1, 1 << 31):
        with pytest.raises(ValueError, match="capacity"):
            metrics.basin_saddles(dh, dl, dl, capacity=cap)


def test_too_many_basins_names_the_remedies(monkeypatch):
    dh, dl = _pretend(torch.zeros((4, 5, 6))), _pretend(torch.zeros((4, 5, 6), dtype=torch.int32))
    monkeypatch.setattr(metrics, "basins", lambda *a, **kw: (None, 11))
    monkeypatch.setattr(metrics, "basin_saddles", lambda *a, **kw: pytest.fail("went on past the refusal"))
    with pytest.raises(ValueError) as e:
        metrics.split_components(dl, dh, 1.0, max_basins=10)
    assert "11 basins" in str(e.value) and "smooth" in str(e.value) and "prominence" in str(e.value)


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


def test_script_defaults_split_nothing():
    mod = _script()
    parser = mod.create_argparser()
    args = parser.parse_args([])
    assert args.roi_split_prominence is None and args.roi_split_fwhm == 0.0
    assert mod._check_split(parser, args) is None


def _files(tmp_path):
    shape = (12, 16, 24)
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.ones(shape, dtype=np.float32))
    lab = np.zeros(shape, dtype=np.int32)
    lab[2:5, 3:6, 4:9] = 3
    np.save(tmp_path / "lab.npy", lab)
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path),
            "--target_samples", str(tmp_path / "full.npz")]


SEG = ["--roi_threshold", "0.5"]
SPACING = ["--voxel_spacing", "2", "2", "2"]
CASES = {
    "zero": (SEG + ["--roi_split_prominence", "0"], "--roi_split_prominence"),
    "negative": (SEG + ["--roi_split_prominence", "-0.5"], "--roi_split_prominence"),
    "nan": (SEG + ["--roi_split_prominence", "nan"], "--roi_split_prominence"),
    "inf": (SEG + ["--roi_split_prominence", "inf"], "--roi_split_prominence"),
    "no_threshold": (["--roi_split_prominence", "0.5"], "--roi_threshold"),
    "with_labels": (["--roi_labels", "LAB", "--roi_split_prominence", "0.5"], "--roi_labels"),
    "fwhm_alone": (SEG + SPACING + ["--roi_split_fwhm", "4"], "--roi_split_prominence"),
    "fwhm_negative": (SEG + SPACING + ["--roi_split_prominence", "0.5", "--roi_split_fwhm", "-1"], "--roi_split_fwhm"),
    "fwhm_nan": (SEG + SPACING + ["--roi_split_prominence", "0.5", "--roi_split_fwhm", "nan"], "--roi_split_fwhm"),
    "fwhm_no_spacing": (SEG + ["--roi_split_prominence", "0.5", "--roi_split_fwhm", "4"], "--voxel_spacing"),
    "fwhm_radius": (SEG + SPACING + ["--roi_split_prominence", "0.5", "--roi_split_fwhm", "40"], "--roi_split_fwhm"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_script_refuses_bad_split_flags_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, names = CASES[case]
    argv = _files(tmp_path) + [str(tmp_path / "lab.npy") if a == "LAB" else a for a in extra]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    assert names in capsys.readouterr().err


@pytest.mark.parametrize("flags", [SEG + ["--roi_split_prominence", "0.5"],
                                   SEG + SPACING + ["--roi_split_prominence", "0.5", "--roi_split_fwhm", "4"]],
                         ids=["raw", "smoothed"])
def test_script_accepts_good_flags_before_it_builds_the_model(flags, tmp_path, monkeypatch):
    """the same set-up with nothing wrong reaches the first device call: the refusals above are the checks' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path) + flags)
