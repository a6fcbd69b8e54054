"""
GPU tier of the distance transform and the lesion boundary figures: ddpm3d_distance_sq and
metrics.distance_sq against the yardstick (tests/edt_ref.py) on volumes whose shape is derived from the kernel's
column group C and its limit MAX, so that they cross a column group and a wave along every axis: equality at unit
spacing, the 5-rounding bound at three anisotropic spacings, degenerate shapes up to the limit, the limit + 1, all
foreground and all background, invert, mask values, independence of the stack and of what the buffers held before,
bit-repeatability; surface, boundary and edge_profile against their restatements, the empty estimate, one
device-to-host copy per boundary call; and the inference script's --roi_boundary and --roi_edge_profile_mm on two of
its paths.
"""

import functools
import importlib.util
import json
import os
import warnings

import numpy as np
import pytest
import torch

import edt_ref as R
from conftest import PKG
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

C, MAX = _hip.EDT_COLUMNS, _hip.EDT_MAX_EXTENT
SHAPE = (67, 2 * C + 3, 130)            # two waves and a tail along W; two column groups and a tail along H, and of H * W
DENSITIES = (0.5, 0.9, 0.99, 0.999)
UNIT = (1.0, 1.0, 1.0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # a copy: the cached masks are read-only


@functools.lru_cache(maxsize=None)
def mask_of(density):
    m = R.random_mask(SHAPE, density, seed=int(density * 1000))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def want_of(density, spacing):
    w = R.distance_sq(mask_of(density), spacing)
    w.setflags(write=False)
    return w


def raw(mask, spacing, invert=0, fill=None):
    """the C entry itself on a (K, D, H, W) or (D, H, W) uint8 array -> float32 array; `fill` pre-sets out's bytes"""
    lib = _hip.load()
    m = dev(mask)
    K = mask.shape[0] if mask.ndim == 4 else 1
    D, H, W = mask.shape[-3:]
    out = torch.empty(mask.shape, dtype=torch.float32, device="cuda")
    if fill is not None:
        out.view(torch.uint8).fill_(fill)
    _hip.check(lib.ddpm3d_distance_sq(_hip.ptr(m), K, D, H, W, invert, spacing[0], spacing[1], spacing[2],
                                      _hip.ptr(out), _hip.stream()))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("density", DENSITIES)
def test_unit_spacing_is_exact(density):
    got = metrics.distance_sq(dev(mask_of(density)), UNIT)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == SHAPE
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want_of(density, UNIT))
    assert np.array_equal(raw(mask_of(density), UNIT), got.cpu().numpy())


@pytest.mark.parametrize("spacing", R.SPACINGS, ids=str)
def test_anisotropic_spacings_hold_the_bound(spacing, capsys):
    shares = []
    for density in DENSITIES:
        got = metrics.distance_sq(dev(mask_of(density)), spacing).cpu().numpy()
        shares.append(R.share_of_bound(got, want_of(density, spacing)))
    with capsys.disabled():
        print("\ndistance_sq at %s, densities %s: %s of the bound" % (spacing, DENSITIES,
                                                                      ", ".join("%.3f" % s for s in shares)))
    assert max(shares) <= 1.0, shares


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, MAX), (MAX, 1, 3), (1, MAX, 2)], ids=str)
@pytest.mark.parametrize("end", [0, -1], ids=["first", "last"])
def test_degenerate_shapes_with_one_background_voxel_at_an_end(shape, end):
    mask = np.ones(shape, dtype=np.uint8)
    mask.reshape(-1)[end] = 0
    got = raw(mask, UNIT).astype(np.float64)
    want = R.distance_sq(mask, UNIT)
    assert np.array_equal(got, want) and np.array_equal(want, np.rint(want))
    assert want.max() >= (max(shape) - 1) ** 2


def test_the_limit_plus_one_is_refused():
    lib = _hip.load()
    for shape in ((1, 1, MAX + 1), (1, MAX + 1, 1), (MAX + 1, 1, 1)):
        m = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="every extent is at most %d" % MAX):
            metrics.distance_sq(m, UNIT)
        out = torch.empty(shape, dtype=torch.float32, device="cuda")
        rc = lib.ddpm3d_distance_sq(_hip.ptr(m), 1, shape[0], shape[1], shape[2], 0, 1.0, 1.0, 1.0, _hip.ptr(out),
                                    _hip.stream())
        assert rc == _hip.E_INVAL and lib.ddpm3d_last_error().decode().startswith("distance_sq:")


def test_all_foreground_all_background_invert_and_mask_values():
    ones = np.ones(SHAPE, dtype=np.uint8)
    assert np.array_equal(raw(ones, (3.27, 2.0, 2.0)), np.full(SHAPE, np.inf, dtype=np.float32))
    assert not raw(0 * ones, (3.27, 2.0, 2.0)).any()
    assert not raw(ones, (3.27, 2.0, 2.0), invert=1).any()
    m = mask_of(0.9)
    spacing = R.SPACINGS[1]
    plain = raw(m, spacing)
    assert np.array_equal(raw(1 - m, spacing, invert=1).view(np.uint32), plain.view(np.uint32))
    mixed = np.where(m != 0, np.where(R.random_mask(SHAPE, 0.5, seed=1) != 0, 255, 1), 0).astype(np.uint8)
    assert np.array_equal(raw(mixed, spacing).view(np.uint32), plain.view(np.uint32))
    as_bool = metrics.distance_sq(dev(m != 0), spacing)
    assert np.array_equal(as_bool.cpu().numpy().view(np.uint32), plain.view(np.uint32))
    # the complement's transform is the yardstick's with invert
    assert R.share_of_bound(raw(m, spacing, invert=1), R.distance_sq(m, spacing, invert=True)) <= 1.0


def test_a_stack_is_its_volumes_whatever_the_buffers_held():
    spacing = R.SPACINGS[0]
    stack = np.stack([mask_of(0.5), mask_of(0.99), np.ones(SHAPE, dtype=np.uint8)])
    singles = np.stack([raw(m, spacing, fill=0xFF) for m in stack])
    both = raw(stack, spacing, fill=0xFF)
    assert np.array_equal(both.view(np.uint32), singles.view(np.uint32))
    assert np.array_equal(raw(stack, spacing, fill=0x00).view(np.uint32), both.view(np.uint32))
    again = metrics.distance_sq(dev(stack), spacing).cpu().numpy()
    assert again.shape == stack.shape and np.array_equal(again.view(np.uint32), both.view(np.uint32))


# ------------------------------------------------------------------------------------------ the consumers
SPACING = (3.0, 2.0, 2.0)


def close(got, want, bound=R.BOUND_MM):
    return got is not None and want is not None and abs(got - want) <= bound * abs(want)


def test_surface_is_the_yardsticks():
    t, e, _, _ = R.blobs()
    for labels in (t, e, np.ones_like(t), 0 * t):
        got = metrics.surface(dev(labels > 0))
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), R.surface(labels > 0))
    m = mask_of(0.9)
    assert np.array_equal(metrics.surface(dev(m)).cpu().numpy(), R.surface(m))


def test_boundary_against_the_yardstick(capsys):
    t, e, _, _ = R.blobs()
    want, sets = R.boundary(t, e, SPACING)
    # the percentiles are taken over identical voxel sets
    assert np.array_equal(metrics.surface(dev(t > 0)).cpu().numpy(), R.surface(t > 0))
    assert np.array_equal(metrics.surface(dev(e > 0)).cpu().numpy(), R.surface(e > 0))
    got = metrics.boundary(dev(t), dev(e), SPACING)
    assert set(got) == set(want) and list(got["regions"]) == [1, 2]
    for key in ("dice", "jaccard", "n_surface_target", "n_surface_estimate"):
        assert got[key] == want[key], key
    shares = []
    for key in ("hd_mm", "hd95_mm", "assd_mm"):
        assert close(got[key], want[key]), (key, got[key], want[key])
        shares.append(abs(got[key] - want[key]) / want[key] / R.BOUND_MM)
    for label in (1, 2):
        assert set(got["regions"][label]) == {"surface_mean_mm", "surface_p95_mm", "surface_max_mm"}
        for key, g in got["regions"][label].items():
            assert close(g, want["regions"][label][key]), (label, key, g, want["regions"][label][key])
            shares.append(abs(g - want["regions"][label][key]) / want["regions"][label][key] / R.BOUND_MM)
    with capsys.disabled():
        print("\nboundary figures: at most %.3f of the bound" % max(shares))
    # the target's side handed in: the same figures
    index = metrics.boundary_target(dev(t), SPACING)
    assert metrics.boundary(dev(t), dev(e), SPACING, index=index) == got
    same = metrics.boundary(dev(t), dev(t), SPACING, index=index)
    assert same["dice"] == 1.0 and same["hd_mm"] == 0.0 and same["hd95_mm"] == 0.0 and same["assd_mm"] == 0.0


def test_boundary_of_an_empty_estimate():
    t, _, _, _ = R.blobs()
    got = metrics.boundary(dev(t), dev(0 * t), SPACING)
    want, _ = R.boundary(t, 0 * t, SPACING)
    assert got == want
    assert got["dice"] == 0.0 and got["hd_mm"] is None and got["hd95_mm"] is None and got["assd_mm"] is None
    assert got["n_surface_estimate"] == 0 and got["regions"][2]["surface_p95_mm"] is None
    with pytest.raises(ValueError, match="the target has no foreground"):
        metrics.boundary(dev(0 * t), dev(t), SPACING)


def test_boundary_makes_one_device_to_host_copy():
    """under torch's sync debug mode every blocking call warns: with the target's side handed in, boundary makes one,
    the copy of its figures"""
    t, e, _, _ = R.blobs()
    tl, el = dev(t), dev(e)
    index = metrics.boundary_target(tl, SPACING)
    metrics.boundary(tl, el, SPACING, index=index)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            metrics.boundary(tl, el, SPACING, index=index)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    blocking = [w for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(blocking) == 1, [str(w.message) for w in seen]


def test_edge_profile_against_the_yardstick():
    """spacing 2 mm and 2.5 mm shells: the CPU tier shows no voxel of the yardstick near a shell edge, so the shells'
    voxel sets are the yardstick's and the means are fixed-order fp64 sums of the same values"""
    t, _, vol, est = R.blobs()
    keep = np.ones(t.shape, dtype=np.uint8)
    keep[:, :, :9] = 0
    for kw, k in ((dict(inside=3, outside=3), None), (dict(inside=2, outside=3), keep), (dict(inside=0, outside=2), None)):
        want = R.edge_profile({"target": vol, "estimate": est}, t, (2.0, 2.0, 2.0), 2.5, keep=k, **kw)
        got = metrics.edge_profile({"target": dev(vol), "estimate": dev(est)}, dev(t), (2.0, 2.0, 2.0), 2.5,
                                   keep=None if k is None else dev(k), **kw)
        assert set(got) == set(want) and len(got["rows"]) == kw["inside"] + kw["outside"]
        assert [(r["distance_mm"], r["n"]) for r in got["rows"]] == [(r["distance_mm"], r["n"]) for r in want["rows"]]
        for g, w in zip(got["rows"], want["rows"]):
            assert g["n"] > 0
            for name in ("target", "estimate"):
                assert g["mean"][name] == pytest.approx(w["mean"][name], rel=1e-12)
    with pytest.raises(ValueError, match="65 shells"):
        metrics.edge_profile({"target": dev(vol)}, dev(t), (2.0, 2.0, 2.0), 2.5, inside=32, outside=33)
    with pytest.raises(ValueError, match="width_mm must be a positive"):
        metrics.edge_profile({"target": dev(vol)}, dev(t), (2.0, 2.0, 2.0), 0.0)
    # shells too thin to hold a voxel, and a volume without a boundary: rows without voxels
    thin = metrics.edge_profile({"target": dev(vol)}, dev(t), (2.0, 2.0, 2.0), 0.5, inside=1, outside=1)
    assert [r["n"] for r in thin["rows"]] == [0, 0] and thin["rows"][0]["mean"]["target"] is None


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _strip(rep):
    """the metrics file without what the two flags add"""
    roi = rep["roi"]
    roi["labels"] = roi["labels"].replace(os.sep + "edges" + os.sep, os.sep + "plain" + os.sep)   # the save_dir
    roi.pop("boundary")
    roi.pop("edge_profile")
    for r in roi["regions"].values():
        r["input"].pop("boundary")
        r["denoised"].pop("boundary")
    return rep


@pytest.mark.parametrize("extra,draws", [([], 0), (["--joint_patches", "True", "--num_draws", "2"], 2)],
                         ids=["one-shot", "joint-draws"])
def test_script_writes_boundary_and_edge_profile(extra, draws, tmp_path):
    import metrics_ref
    import segment_ref as S
    target = metrics_ref.phantom((20, 40, 40), seed=4)                      # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = metrics_ref.noisy(target, 0.1, seed=4)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    mod = _script()
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz"),
                      "--roi_threshold_frac", "0.5", "--roi_min_voxels", "5", "--voxel_spacing", "2", "2", "2"] + extra
    plain_path = mod.main(common + ["--save_dir", str(tmp_path / "plain")])
    path = mod.main(common + ["--save_dir", str(tmp_path / "edges"), "--roi_boundary", "True",
                              "--roi_edge_profile_mm", "2.5"])
    assert open(path, "rb").read() == open(plain_path, "rb").read()         # the written volume does not change
    plain_text = open(tmp_path / "plain" / "metrics_pet.json").read()
    rep = json.load(open(tmp_path / "edges" / "metrics_pet.json"))
    roi = rep["roi"]
    assert {"boundary", "edge_profile", "detection"} <= set(roi)
    plain = json.loads(plain_text)["roi"]
    assert "boundary" not in plain and "edge_profile" not in plain
    assert all("boundary" not in r["input"] and "boundary" not in r["denoised"] for r in plain["regions"].values())

    arr = np.load(path)["arr_0"]                                            # (H, W, Z)
    tgt, inp = np.ascontiguousarray(target.transpose(1, 2, 0)), np.ascontiguousarray(low.transpose(1, 2, 0))
    keep = None
    if not draws:                                                           # Hann weight 0: the outermost planes
        keep = np.zeros(arr.shape, dtype=np.uint8)
        keep[1:-1, 1:-1, 1:-1] = 1
    threshold = float(np.float32(0.5 * float(target.max())))
    want_labels, n = S.segment(tgt, threshold, 26, 5, keep)
    assert n >= 3
    spacing = (2.0, 2.0, 2.0)
    assert set(roi["boundary"]) == {"input", "denoised"}
    for name, vol in (("input", inp), ("denoised", arr)):
        want, _ = R.boundary(want_labels, S.segment(vol, threshold, 26, 5, keep)[0], spacing)
        got = roi["boundary"][name]
        assert set(got) - {"draws"} == set(want) - {"regions"}
        for key in ("dice", "jaccard", "n_surface_target", "n_surface_estimate"):
            assert got[key] == want[key], (name, key)
        for key in ("hd_mm", "hd95_mm", "assd_mm"):
            assert (got[key] is None and want[key] is None) or close(got[key], want[key]) or got[key] == want[key]
        for v in range(1, n + 1):
            figures = roi["regions"][str(v)][name]["boundary"]
            for key, w in want["regions"][v].items():
                assert (figures[key] is None and w is None) or figures[key] == w or close(figures[key], w)
    assert 0.0 < roi["boundary"]["input"]["dice"] <= 1.0
    if draws:
        assert len(roi["boundary"]["denoised"]["draws"]) == draws
        assert all(set(d) == {"dice", "hd95_mm"} and 0.0 <= d["dice"] <= 1.0 for d in roi["boundary"]["denoised"]["draws"])
    else:
        assert "draws" not in roi["boundary"]["denoised"]

    prof = roi["edge_profile"]
    want = R.edge_profile({"target": tgt, "input": inp, "denoised": arr}, want_labels, spacing, 2.5, keep=keep)
    assert (prof["width_mm"], prof["inside"], prof["outside"]) == (2.5, 3, 5) and len(prof["rows"]) == 8
    for g, w in zip(prof["rows"], want["rows"]):
        assert g["distance_mm"] == w["distance_mm"] and g["n"] == w["n"] and set(g["mean"]) == set(w["mean"])
        for k in w["mean"]:
            assert g["mean"][k] == pytest.approx(w["mean"][k], rel=1e-6)
    means = [r["mean"]["target"] for r in prof["rows"] if r["n"]]
    assert means[0] > means[-1]                                             # hotter inside the lesions than around them
    # without the flags the file is what it was: the flags only add their keys
    assert json.dumps(_strip(rep), indent=2) == plain_text


def test_script_edge_profile_from_a_label_file(tmp_path):
    """--roi_labels with --roi_background: that region is not foreground of the profile, and no boundary block"""
    import metrics_ref
    import segment_ref as S
    target = metrics_ref.phantom((20, 40, 40), seed=4)
    low = metrics_ref.noisy(target, 0.1, seed=4)
    labels, n = S.segment(target, float(np.float32(0.5 * float(target.max()))), 26, 5)
    labels[1:4, 1:4, 1:4] = n + 1                                           # a reference region in a corner
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    np.savez(tmp_path / "labels.npz", labels)
    path = _script().main(FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples",
                                   str(tmp_path / "full.npz"), "--roi_labels", str(tmp_path / "labels.npz"),
                                   "--roi_background", str(n + 1), "--voxel_spacing", "2", "2", "2",
                                   "--roi_edge_profile_mm", "2.5", "--save_dir", str(tmp_path / "out")])
    roi = json.load(open(tmp_path / "out" / "metrics_pet.json"))["roi"]
    assert "boundary" not in roi and roi["background"] == n + 1
    arr = np.load(path)["arr_0"]                                            # (H, W, Z)
    hwz = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0))
    keep = np.zeros(arr.shape, dtype=np.uint8)
    keep[1:-1, 1:-1, 1:-1] = 1
    lesions = np.where(labels == n + 1, 0, labels)
    want = R.edge_profile({"target": hwz(target), "input": hwz(low), "denoised": arr}, hwz(lesions), (2.0, 2.0, 2.0),
                          2.5, keep=keep)
    got = roi["edge_profile"]
    assert [(r["distance_mm"], r["n"]) for r in got["rows"]] == [(r["distance_mm"], r["n"]) for r in want["rows"]]
    for g, w in zip(got["rows"], want["rows"]):
        for k in w["mean"]:
            assert g["mean"][k] == pytest.approx(w["mean"][k], rel=1e-6)
