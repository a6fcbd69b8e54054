"""
GPU tier of the lesion segmentation: ddpm3d_label_components and metrics.label_components against
scipy.ndimage.label (tests/segment_ref.py), bit for bit, on volumes whose shapes are derived from the kernel's brick
so that they cross brick borders along every axis: random volumes just below the percolation threshold of each
lattice and well above it, degenerate shapes, all foreground, all background, a serpentine through every brick, the
checkerboard, voxel pairs that touch only across a brick corner or edge, NaN and threshold-valued voxels, a keep
mask; the status words, the root count across flatten workgroups, a short or missing workspace refused with every
buffer untouched, independence of what the buffers held before, bit-repeatability; segment and detection
against the yardstick; one device-to-host copy per detection; and the inference script's --roi_threshold_frac on
two of its paths.  The labelling has one right answer: every comparison is equality.
"""

import importlib.util
import json
import os
import warnings

import numpy as np
import pytest
import torch

import segment_ref as S
from conftest import PKG
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

TD, TH, TW = _hip.CCL_TILE
SHAPE = (2 * TD + 3, 2 * TH + 1, 2 * TW + 5)
CONNECTIVITIES = (6, 18, 26)
CRITICAL = {6: 0.30, 18: 0.14, 26: 0.10}          # site densities just below each lattice's percolation threshold


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def volume_of(mask):
    """fp32 volume whose voxels above 0.5 are the mask"""
    return np.where(mask, 1.0, 0.0).astype(np.float32)


def raw(vol, threshold, connectivity, keep=None, fill=None):
    """the C entry itself -> (roots, status) on the host; `fill` pre-sets every byte of roots, ws and status"""
    lib = _hip.load()
    x = dev(vol)
    k = None if keep is None else dev(keep)
    D, H, W = vol.shape
    need = lib.ddpm3d_label_components_workspace_bytes(D, H, W)
    assert need >= 16 and need % 16 == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    roots = torch.empty((D, H, W), dtype=torch.int32, device="cuda")
    status = torch.empty(2, dtype=torch.int32, device="cuda")
    if fill is not None:
        ws.fill_(fill)
        roots.view(torch.uint8).fill_(fill)
        status.view(torch.uint8).fill_(fill)
    _hip.check(lib.ddpm3d_label_components(_hip.ptr(x), _hip.ptr(k), threshold, connectivity, D, H, W,
                                           _hip.ptr(roots), _hip.ptr(ws), need, _hip.ptr(status), _hip.stream()))
    return roots.cpu().numpy(), status.cpu().tolist()


def check(vol, connectivity, threshold=0.5, keep=None):
    """roots, status, labels and n of one volume against the yardstick; -> n"""
    want, n = S.label(S.foreground(vol, threshold, keep), connectivity)
    roots, status = raw(vol, threshold, connectivity, keep)
    assert status == [0, n], (status, n)
    assert roots.dtype == np.int32 and np.array_equal(roots, S.roots(want))
    labels, got_n = metrics.label_components(dev(vol), threshold, connectivity=connectivity,
                                             keep=None if keep is None else dev(keep))
    assert got_n == n and labels.dtype == torch.int32 and labels.is_cuda and tuple(labels.shape) == vol.shape
    assert np.array_equal(labels.cpu().numpy(), want)
    return n


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("density", ["critical", 0.5, 0.6])
def test_random_volumes(connectivity, density):
    p = CRITICAL[connectivity] if density == "critical" else density
    mask = S.random_mask(SHAPE, p, seed=connectivity)
    n = check(volume_of(mask), connectivity)
    sizes = np.bincount(S.label(mask, connectivity)[0].reshape(-1))[1:]
    print("connectivity %d, density %.2f on %s: %d components, the largest of %d voxels"
          % (connectivity, p, SHAPE, n, sizes.max()))
    assert n >= 1


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 3 * TW + 1), (TD + 1, 1, 1)], ids=str)
def test_degenerate_shapes(shape, connectivity):
    assert check(np.ones(shape, dtype=np.float32), connectivity) == 1
    assert check(np.zeros(shape, dtype=np.float32), connectivity) == 0
    check(volume_of(S.random_mask(shape, 0.5, seed=5)), connectivity)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_all_foreground_and_all_background(connectivity):
    assert check(np.ones(SHAPE, dtype=np.float32), connectivity) == 1
    assert check(np.zeros(SHAPE, dtype=np.float32), connectivity) == 0
    roots, status = raw(np.zeros(SHAPE, dtype=np.float32), 0.5, connectivity)
    assert status == [0, 0] and (roots == -1).all()


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_serpentine_through_every_brick(connectivity):
    mask = S.serpentine(SHAPE)
    for bz in range(0, SHAPE[0], TD):                                       # it does visit every brick
        for by in range(0, SHAPE[1], TH):
            for bx in range(0, SHAPE[2], TW):
                assert mask[bz:bz + TD, by:by + TH, bx:bx + TW].any()
    assert check(volume_of(mask), connectivity) == 1


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_checkerboard(connectivity):
    mask = S.checkerboard(SHAPE)
    assert check(volume_of(mask), connectivity) == (int(mask.sum()) if connectivity == 6 else 1)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_pairs_across_a_brick_corner_and_edge(connectivity):
    corner = np.zeros(SHAPE, dtype=bool)
    corner[TD - 1, TH - 1, TW - 1] = corner[TD, TH, TW] = True
    assert check(volume_of(corner), connectivity) == (1 if connectivity == 26 else 2)
    anti = np.zeros(SHAPE, dtype=bool)                                      # the other diagonal of the same corner
    anti[TD - 1, TH, TW - 1] = anti[TD, TH - 1, TW] = True
    assert check(volume_of(anti), connectivity) == (1 if connectivity == 26 else 2)
    for a, b in (((TD - 1, TH - 1, 3), (TD, TH, 3)), ((TD - 1, 3, TW - 1), (TD, 3, TW)),
                 ((3, TH - 1, TW - 1), (3, TH, TW)), ((3, TH, TW - 1), (3, TH - 1, TW)),
                 ((TD, 3, TW - 1), (TD - 1, 3, TW)), ((TD, TH - 1, 3), (TD - 1, TH, 3))):
        edge = np.zeros(SHAPE, dtype=bool)
        edge[a] = edge[b] = True
        assert check(volume_of(edge), connectivity) == (2 if connectivity == 6 else 1), (a, b)
    for a, b in (((TD - 1, 2, 2), (TD, 2, 2)), ((2, TH - 1, 2), (2, TH, 2)), ((2, 2, TW - 1), (2, 2, TW))):
        face = np.zeros(SHAPE, dtype=bool)
        face[a] = face[b] = True
        assert check(volume_of(face), connectivity) == 1, (a, b)


def test_nan_and_threshold_valued_voxels_are_background():
    vol = np.full(SHAPE, 2.5, dtype=np.float32)                             # all at the threshold: nothing above it
    assert check(vol, 26, threshold=2.5) == 0
    vol[3:6, 3:6, TW - 2:TW + 2] = np.float32(2.5000002)                    # the next fp32 above 2.5
    vol[4, 4, TW - 1:TW + 1] = np.nan                                       # a hole, not a bridge
    vol[10, 10, 10:20] = 3.0
    vol[10, 10, 15] = np.nan                                                # cuts the line in two
    vol[14, 3, 3] = np.inf
    assert check(vol, 6, threshold=2.5) == 4
    assert check(vol, 26, threshold=2.5) == 4
    assert check(vol, 26, threshold=-np.inf) == 1                           # everything but the NaNs


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_keep_cuts_a_component_in_two(connectivity):
    vol = np.zeros(SHAPE, dtype=np.float32)
    vol[2:TD + 4, 5, 5] = 1.0                                               # a line across a brick border along D
    vol[12, TH - 3:TH + 3, TW - 3:TW + 3] = 1.0                             # a plate over a brick corner
    keep = np.ones(SHAPE, dtype=np.uint8)
    assert check(vol, connectivity, keep=keep) == 2
    keep[TD, 5, 5] = 0                                                      # the line's first voxel beyond the border
    keep[12, TH - 3:TH + 3, TW] = 0                                         # a column of the plate
    keep[0, 0, 0] = 0
    assert check(vol, connectivity, keep=keep) == 4
    keep[:] = 0
    assert check(vol, connectivity, keep=keep) == 0
    keep[:] = 255
    assert check(vol, connectivity, keep=keep) == 2


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_result_does_not_depend_on_what_the_buffers_held(connectivity):
    vol = volume_of(S.random_mask(SHAPE, CRITICAL[connectivity], seed=40 + connectivity))
    first = raw(vol, 0.5, connectivity)
    again = raw(vol, 0.5, connectivity)
    filled = raw(vol, 0.5, connectivity, fill=0x7f)
    assert first[1] == again[1] == filled[1] and first[1][0] == 0
    assert first[0].tobytes() == again[0].tobytes() == filled[0].tobytes()


def test_a_short_or_missing_workspace_is_refused():
    """the need: the 16-byte status accumulator and one count word per 1024 voxels (the flatten's workgroups), not
    the constant 16 bytes first planned: the labelling flatten measured slower with its counts in the accumulator"""
    lib = _hip.load()
    size = lib.ddpm3d_label_components_workspace_bytes
    need = size(*SHAPE)
    for shape in ((1, 1, 1), SHAPE):
        voxels = shape[0] * shape[1] * shape[2]
        assert size(*shape) % 16 == 0 and 16 < size(*shape) <= 16 + 16 + 4 * (voxels // 1024), shape
    assert size(0, 4, 4) == size(4, 0, 4) == size(4, 4, 0) == 0
    x = dev(volume_of(S.random_mask(SHAPE, 0.5, seed=1)))
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device="cuda")
    roots = torch.full(SHAPE, -77, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    for ws_ptr, ws_bytes in ((_hip.ptr(ws), need - 1), (None, need)):
        rc = lib.ddpm3d_label_components(_hip.ptr(x), None, 0.5, 26, *SHAPE, _hip.ptr(roots), ws_ptr, ws_bytes,
                                         _hip.ptr(status), _hip.stream())
        assert rc == _hip.E_INVAL, (rc, ws_bytes)
        assert lib.ddpm3d_last_error().decode().startswith("label_components: needs %d bytes" % need)
        torch.cuda.synchronize()
        assert bool((roots == -77).all()) and status.tolist() == [-7, -7] and bool((ws == 0x5a).all())


def test_root_count_across_flatten_workgroups():
    """every foreground voxel of the 6-connected checkerboard is its own root, so every flatten workgroup (several,
    the last one ragged) adds its share of the count; the number is numpy's"""
    shape = (TD + 1, TH + 1, 2 * TW + 1)
    mask = S.checkerboard(shape)
    roots, status = raw(volume_of(mask), 0.5, 6, fill=0x7f)
    assert status == [0, int(mask.sum())] and int(mask.sum()) > 4 * 1024
    flat = np.arange(mask.size, dtype=np.int32).reshape(shape)
    assert np.array_equal(roots, np.where(mask, flat, -1))


def test_python_entry_refuses_what_it_cannot_take():
    x = torch.zeros(SHAPE, device="cuda")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.label_components(x.cpu(), 0.5)
    with pytest.raises(RuntimeError, match="float32"):
        metrics.label_components(x.double(), 0.5)
    with pytest.raises(ValueError):
        metrics.label_components(x[0], 0.5)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.label_components(x, 0.5, connectivity=8)
    with pytest.raises(ValueError, match="NaN"):
        metrics.label_components(x, float("nan"))
    with pytest.raises(ValueError, match="keep"):
        metrics.label_components(x, 0.5, keep=torch.ones(SHAPE, device="cuda"))
    with pytest.raises(ValueError, match="keep"):
        metrics.label_components(x, 0.5, keep=torch.ones(SHAPE[1:], dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------ segment, detection
@pytest.mark.parametrize("min_voxels", [1, 2, 50])
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_segment_equals_the_yardstick(connectivity, min_voxels):
    rng = np.random.default_rng(7)
    vol = rng.random(SHAPE, dtype=np.float32)
    threshold = 1.0 - CRITICAL[connectivity]
    keep = (rng.random(SHAPE) < 0.97).astype(np.uint8)
    for k in (None, keep):
        want, n = S.segment(vol, threshold, connectivity, min_voxels, k)
        labels, got_n = metrics.segment(dev(vol), threshold, connectivity=connectivity, min_voxels=min_voxels,
                                        keep=None if k is None else dev(k))
        assert got_n == n and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want)
    assert n > 0
    none, zero = metrics.segment(dev(vol), threshold, connectivity=connectivity, min_voxels=vol.size)
    assert zero == 0 and not none.any()


def test_detection_equals_the_yardstick():
    t, e = S.blobs_pair()
    tl, nt = metrics.segment(dev(t), 1.0)
    el, ne = metrics.segment(dev(e), 1.0)
    assert (nt, ne) == (5, 7)
    got = metrics.detection(tl, el)
    assert got == S.detection(S.segment(t, 1.0)[0], S.segment(e, 1.0)[0])
    assert (got["n_found"], got["n_missed"], got["false_positives"]) == (4, 1, 2)
    assert got["found"] == [False, True, True, True, True] and got["sensitivity"] == 0.8
    back = metrics.detection(el, tl)                                        # the roles swapped
    assert back == S.detection(S.segment(e, 1.0)[0], S.segment(t, 1.0)[0])
    empty = torch.zeros_like(tl)
    assert metrics.detection(empty, el) == S.detection(np.zeros(t.shape, dtype=np.int32), S.segment(e, 1.0)[0])
    assert metrics.detection(tl, empty)["n_missed"] == 5
    dots = np.zeros(SHAPE, dtype=np.float32)                                # many estimate components: no cap on them
    dots[::2, ::2, ::2] = 1.0
    noise = np.random.default_rng(11).random(SHAPE, dtype=np.float32)
    many, n_many = metrics.segment(dev(dots), 0.5, connectivity=26)
    few, n_few = metrics.segment(dev(noise), 0.6, connectivity=26, min_voxels=300)
    assert n_many == dots.sum() > _hip.ROI_MAX_REGIONS and n_few == 1
    assert metrics.detection(few, many) == S.detection(S.segment(noise, 0.6, 26, 300)[0], S.segment(dots, 0.5)[0])
    with pytest.raises(ValueError, match="target regions"):
        metrics.detection(many, few)
    with pytest.raises(ValueError):
        metrics.detection(tl, el[:, :, :-1])
    with pytest.raises(ValueError, match="integer"):
        metrics.detection(tl.float(), el)


def test_detection_makes_one_device_to_host_copy():
    """under torch's sync debug mode every blocking call warns: detection makes one, the copy of its counts"""
    t, e = S.blobs_pair()
    tl, el = metrics.segment(dev(t), 1.0)[0], metrics.segment(dev(e), 1.0)[0]
    metrics.detection(tl, el)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            metrics.detection(tl, el)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    blocking = [w for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(blocking) == 1, [str(w.message) for w in seen]


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
ONLY_HERE = {"found", "overlap"}
DRAW_KEYS = {"draw_means", "mean_std", "mean_z"}


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _without(d, keys):
    return {k: v for k, v in d.items() if k not in keys}


@pytest.mark.parametrize("extra,draws,seg", [
    ([], 0, dict(frac=0.5, connectivity=26, min_voxels=5)),
    (["--patch_overlap", "4", "--num_draws", "2"], 2, dict(frac=0.4, connectivity=6, min_voxels=1)),
], ids=["one-shot", "sliding-draws"])
def test_script_segments_the_target(extra, draws, seg, tmp_path, monkeypatch, capsys):
    import metrics_ref
    target = metrics_ref.phantom((20, 40, 40), seed=4)                      # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = metrics_ref.noisy(target, 0.1, seed=4)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    mod = _script()
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz")]
    common += extra
    seg_flags = ["--roi_threshold_frac", str(seg["frac"]), "--roi_connectivity", str(seg["connectivity"]),
                 "--roi_min_voxels", str(seg["min_voxels"])]
    path = mod.main(common + ["--save_dir", str(tmp_path / "seg")] + seg_flags)
    rep = json.load(open(tmp_path / "seg" / "metrics_pet.json"))
    assert set(rep) == {"denoised", "input", "target", "mask_threshold", "roi"}
    roi = rep["roi"]
    assert set(roi) == {"labels", "background", "threshold", "connectivity", "min_voxels", "regions", "detection"}
    threshold = float(np.float32(seg["frac"] * float(target.max())))
    assert roi["threshold"] == threshold and roi["background"] is None
    assert roi["connectivity"] == seg["connectivity"] and roi["min_voxels"] == seg["min_voxels"]
    labels_path = str(tmp_path / "seg" / "roi_labels_pet.npz")
    assert roi["labels"] == labels_path and os.path.isfile(labels_path)

    out = np.load(path)
    arr = out["arr_0"]                                                       # (H, W, Z)
    tgt, inp = np.ascontiguousarray(target.transpose(1, 2, 0)), np.ascontiguousarray(low.transpose(1, 2, 0))
    keep = np.zeros(arr.shape, dtype=np.uint8)                              # Hann weight 0: the outermost planes
    keep[1:-1, 1:-1, 1:-1] = 1
    args = (threshold, seg["connectivity"], seg["min_voxels"], keep)
    want_labels, n = S.segment(tgt, *args)
    assert n >= 3
    written = np.load(labels_path)["arr_0"]
    assert written.dtype == np.int32 and written.shape == target.shape      # (D, H, W), as --roi_labels reads it
    assert np.array_equal(written, want_labels.transpose(2, 0, 1))

    index = metrics.roi_index(dev(want_labels), keep=dev(keep))
    want_den = metrics.roi_report(dev(arr), dev(tgt), index)
    want_inp = metrics.roi_report(dev(inp), dev(tgt), index)
    want_det = {"input": S.detection(want_labels, S.segment(inp, *args)[0]),
                "denoised": S.detection(want_labels, S.segment(arr, *args)[0])}
    assert list(roi["regions"]) == [str(v) for v in range(1, n + 1)]
    for v in range(1, n + 1):
        r = roi["regions"][str(v)]
        assert set(r) == {"n", "target", "input", "denoised"} and r["n"] == int((want_labels == v).sum())
        assert r["target"] == want_den[v]["target"]
        assert _without(r["input"], ONLY_HERE) == want_inp[v]["estimate"]
        assert _without(r["denoised"], ONLY_HERE | DRAW_KEYS) == want_den[v]["estimate"]
        for name in ("input", "denoised"):
            assert r[name]["found"] == want_det[name]["found"][v - 1]
            assert r[name]["overlap"] == want_det[name]["overlap"][v - 1]
        assert bool(DRAW_KEYS & set(r["denoised"])) == bool(draws)
    det = roi["detection"]
    assert set(det) == {"input", "denoised"} and det["input"] == want_det["input"]
    assert _without(det["denoised"], {"draws"}) == want_det["denoised"]
    if draws:
        assert len(det["denoised"]["draws"]) == draws
        for d in det["denoised"]["draws"]:
            assert set(d) == {"n_found", "false_positives"} and 0 <= d["n_found"] <= n and d["false_positives"] >= 0
    else:
        assert "draws" not in det["denoised"]
        # the written labels fed back through --roi_labels: the same regions but for the keys only this path writes
        mod.main(common + ["--save_dir", str(tmp_path / "fed"), "--roi_labels", labels_path])
        fed = json.load(open(tmp_path / "fed" / "metrics_pet.json"))["roi"]
        assert set(fed) == {"labels", "background", "regions"} and list(fed["regions"]) == list(roi["regions"])
        for v, r in roi["regions"].items():
            assert fed["regions"][v] == {"n": r["n"], "target": r["target"], "input": _without(r["input"], ONLY_HERE),
                                         "denoised": _without(r["denoised"], ONLY_HERE)}
        assert open(tmp_path / "fed" / "denoised_pet.npz", "rb").read() == open(path, "rb").read()
        # a threshold above the target's maximum is refused before the first sampling step
        def sampled(*a, **k):
            raise AssertionError("the script went on to sample")

        monkeypatch.setattr(mod, "_sampler", sampled)
        monkeypatch.setattr(mod, "_run_patches", sampled)
        monkeypatch.setattr(mod, "_main_joint", sampled)
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.main(common + ["--save_dir", str(tmp_path / "high"), "--roi_threshold", str(2.0 * float(target.max()))])
        assert e.value.code == 2 and "--roi_min_voxels" in capsys.readouterr().err
        assert not os.path.exists(tmp_path / "high" / "denoised_pet.npz")
