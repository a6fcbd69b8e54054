"""
GPU tier of SUVpeak / MTV / TLG: ddpm3d_sphere_mean through metrics.sphere_mean against the fp64
yardstick of tests/peak_ref.py, every voxel within the entry's own bound (n + 2) 2^-24 (sum |x_i| / n), on volumes
thinner than the footprint, no multiple of the tile, with the largest radius, and on footprints that take each of
the kernel's tile shapes; with and without an offset of 1000, a keep mask with voxels that count nothing, one and
three volumes per call; impulses at a corner, on a face, across a tile border and inside; the single-voxel footprint;
bit-repeatability and independence of B; roi_peak and roi_report with a spacing; and the inference script's
--voxel_spacing on two of its paths.
"""

import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import peak_ref as P
from conftest import PKG
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

# shape, spacing: thinner than the footprint along D and no tile multiple along H and W; anisotropic; the largest
# radius along W; a single row.  Then two footprints with large radii on both slow axes, which take the smallest
# tiles: (4, 4, 3) stages 2 x 4 x 64 (1 x 4 x 64 with keep), (8, 8, 3) one workgroup per CU on 8 x 8 x 64 (4 x 4 x 64).
CASES = [
    ((5, 37, 70), (2.0, 2.0, 2.0)),
    ((19, 21, 67), (3.27, 2.0, 1.5)),
    ((20, 33, 40), (6.0, 2.0, 0.775)),
    ((1, 1, 9), (2.0, 2.0, 2.0)),
    ((11, 13, 66), (1.5, 1.5, 2.0)),
    ((9, 10, 65), (0.775, 0.775, 2.0)),
]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def within_bound(got, ref, what):
    """every voxel of one volume within the bound of the yardstick; prints the largest share of the bound used"""
    mean, n, bound = ref
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - mean)
    used = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s: largest deviation %.3g = %.3f of the bound" % (what, float(err.max()), used))
    assert (err <= bound).all(), (what, float(err.max()), used)
    assert (got[n == 0] == 0.0).all() and not np.signbit(got[n == 0]).any()
    return used


@pytest.mark.parametrize("masked", [False, True], ids=["all", "keep"])
@pytest.mark.parametrize("offset", [0.0, 1000.0], ids=["centred", "offset1000"])
@pytest.mark.parametrize("shape,spacing", CASES, ids=lambda v: "x".join(str(a) for a in v))
def test_every_voxel_within_the_bound(shape, spacing, offset, masked):
    fp = metrics.sphere_footprint(spacing)
    x, keep, ref = P.case(shape, spacing, offset, masked)
    k = None if keep is None else dev(keep)
    if masked:
        assert (ref[0][1] == 0).any()                        # the block of zeros leaves voxels that count nothing
    else:
        assert (ref[0][1] > 0).all() and ref[0][1].max() <= fp.taps
    got = metrics.sphere_mean(dev(x), fp, keep=k)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == shape
    within_bound(got, ref[0], "%s at %s, offset %g, %s, B = 1" % (shape, spacing, offset, "keep" if masked else "all"))
    xs, _, refs = P.case(shape, spacing, offset, masked, batch=3)
    stack = metrics.sphere_mean(dev(xs), fp, keep=k)
    assert tuple(stack.shape) == (3,) + shape
    for b in range(3):
        within_bound(stack[b], refs[b], "  volume %d of 3" % b)


def test_interior_count_is_the_tap_count():
    """a volume with tiles whose whole footprint lies inside: the kernel's constant count against the yardstick's"""
    shape, spacing = (24, 40, 200), (4.0, 4.0, 4.0)
    fp = metrics.sphere_footprint(spacing)
    x, _, ref = P.case(shape, spacing, 0.0, False)
    assert (ref[0][1][1:-1, 1:-1, 1:-1] == 19).all()
    within_bound(metrics.sphere_mean(dev(x), fp), ref[0], "%s at %s" % (shape, spacing))


@pytest.mark.parametrize("masked", [False, True], ids=["all", "keep"])
def test_impulses_give_the_clipped_footprint(masked):
    shape, spacing = (7, 12, 70), (3.27, 2.0, 1.5)            # radii (1, 3, 4): a swapped axis cannot pass
    fp = metrics.sphere_footprint(spacing)
    box, radii = P.trimmed(P.footprint(spacing))
    assert radii == (1, 3, 4)
    keep = np.ones(shape, dtype=np.uint8)
    if masked:
        keep[:, 5, :] = 0
    ones = P.sphere_mean(np.ones(shape), P.footprint(spacing), keep)[1]       # the count around every voxel
    for at in [(0, 0, 0), (6, 11, 69), (3, 0, 40), (0, 6, 30), (3, 6, 30), (3, 6, 64), (3, 4, 63), (6, 8, 2)]:
        x = np.zeros(shape, dtype=np.float32)
        x[at] = 1.0
        got = metrics.sphere_mean(dev(x), fp, keep=dev(keep) if masked else None).cpu().numpy()
        want = np.zeros(shape, dtype=np.float32)
        for off in np.argwhere(box):
            v = tuple(np.array(at) - (off - np.array(radii)))   # the voxels whose footprint holds `at`
            if all(0 <= c < s for c, s in zip(v, shape)):
                want[v] = np.float32(1.0) / np.float32(ones[v])
        assert np.array_equal(got != 0, want != 0), at
        assert np.array_equal(got, want), at


def test_an_unkept_nan_stays_out():
    shape, spacing = (4, 9, 20), (4.0, 4.0, 4.0)
    x = P.data(shape, 3).copy()
    keep = np.ones(shape, dtype=np.uint8)
    x[2, 4, 10] = np.nan
    keep[2, 4, 10] = 0
    got = metrics.sphere_mean(dev(x), metrics.sphere_footprint(spacing), keep=dev(keep))
    assert torch.isfinite(got).all()
    within_bound(got, P.sphere_mean(np.nan_to_num(x), P.footprint(spacing), keep), "unkept NaN")


@pytest.mark.parametrize("masked", [False, True], ids=["all", "keep"])
def test_single_voxel_footprint_copies_the_input(masked):
    shape = (3, 9, 70)
    fp = metrics.sphere_footprint((7.0, 7.0, 7.0))
    assert fp.taps == 1
    x = P.data(shape, 5, offset=0.0).copy()
    x[0, 0, :4] = [0.0, -0.0, np.float32(1e-42), -np.inf]    # signed zeros, a denormal and an infinity keep their bits
    keep = (np.random.default_rng(6).random(shape) < 0.6).astype(np.uint8) if masked else np.ones(shape, np.uint8)
    keep[0, 0, :4] = 1
    got = metrics.sphere_mean(dev(x), fp, keep=dev(keep) if masked else None)
    want = torch.where(dev(keep) != 0, bits(dev(x)), torch.zeros_like(bits(dev(x))))
    assert torch.equal(bits(got), want)


def test_rows_do_not_depend_on_b_and_runs_repeat():
    shape, spacing = (19, 21, 67), (3.27, 2.0, 1.5)
    fp = metrics.sphere_footprint(spacing)
    xs, keep, _ = P.case(shape, spacing, 1000.0, True, batch=3)
    for k in (None, dev(keep)):
        stack = metrics.sphere_mean(dev(xs), fp, keep=k)
        again = metrics.sphere_mean(dev(xs), fp, keep=k)
        assert torch.equal(bits(stack), bits(again))
        for b in range(3):
            assert torch.equal(bits(metrics.sphere_mean(dev(xs[b]), fp, keep=k)), bits(stack[b]))


def test_python_entry_refuses_what_it_cannot_take():
    fp = metrics.sphere_footprint((2.0, 2.0, 2.0))
    x = torch.zeros((4, 5, 6), device="cuda")
    for bad in (torch.zeros((5, 6), device="cuda"), torch.zeros((1, 2, 4, 5, 6), device="cuda")):
        with pytest.raises(ValueError, match="sphere_mean: volume of shape"):
            metrics.sphere_mean(bad, fp)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        metrics.sphere_mean(x.permute(2, 0, 1), fp)
    for keep in (torch.ones((4, 5, 6), dtype=torch.uint8), torch.ones((4, 5, 6), device="cuda"),
                 torch.ones((4, 5, 7), dtype=torch.uint8, device="cuda"),
                 torch.ones((6, 4, 5), dtype=torch.uint8, device="cuda").permute(1, 2, 0)):
        with pytest.raises(ValueError, match="keep must be a contiguous device uint8 tensor"):
            metrics.sphere_mean(x, fp, keep=keep)
    with pytest.raises(ValueError, match="footprint"):
        metrics.sphere_mean(x, (3, 3, 3))
    with pytest.raises(ValueError, match="volumes"):
        metrics.sphere_mean(torch.zeros((_hip.MAX_DRAWS + 1, 1, 1, 2), device="cuda"), fp)


# ------------------------------------------------------------------------------------------ regions
SHAPE, SPACING = (19, 21, 67), (3.27, 2.0, 1.5)


def _regions():
    """five regions: one voxel, one touching a face and a corner, one across the tile border along W, two blobs"""
    lab = np.zeros(SHAPE, dtype=np.int32)
    lab[9, 10, 33] = 1
    lab[0:3, 0:4, 0:6] = 2
    lab[5:9, 8:12, 60:67] = 3
    lab[12:17, 3:9, 20:31] = 4
    lab[10:14, 14:20, 40:52] = 7
    return lab


def _pet(seed, scale=1.0):
    """positive, PET-like: a smooth field times `scale` plus noise, so that peaks of two volumes differ for good"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in SHAPE], indexing="ij")
    field = 1.0 + np.sin(3.0 * z) * np.cos(4.0 * y) * np.sin(5.0 * x + 1.0) ** 2
    return (scale * field + 0.2 * rng.random(SHAPE)).astype(np.float32)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "keep"])
def test_roi_peak_is_the_maximum_of_the_map_over_the_region(masked):
    fp = metrics.sphere_footprint(SPACING)
    lab, x = _regions(), _pet(1)
    keep = None
    if masked:
        keep = (np.random.default_rng(2).random(SHAPE) < 0.7).astype(np.uint8)
        keep[9, 10, 33] = 1                                   # the one-voxel region stays a region
    k = None if keep is None else dev(keep)
    index = metrics.roi_index(dev(lab), keep=k)
    assert index.labels == [1, 2, 3, 4, 7] and index.counts[0] == 1
    peaks = metrics.roi_peak(dev(x), index, fp, keep=k)
    gpu_map = metrics.sphere_mean(dev(x), fp, keep=k).cpu().numpy()
    mean, n, bound = P.sphere_mean(x, P.footprint(SPACING), keep)
    want = P.region_peaks(mean, bound, lab, index.labels, keep)
    for r, v in enumerate(index.labels):
        at = (lab == v) if keep is None else (lab == v) & (keep != 0)
        assert np.float32(peaks[r]) == gpu_map[at].max() and peaks[r] == float(gpu_map[at].max())   # bit for bit
        print("region %d: peak %.7g, yardstick %.7g, bound %.3g" % (v, peaks[r], want[r][0], want[r][1]))
        assert abs(peaks[r] - want[r][0]) <= want[r][1]
    stack = np.stack([x, _pet(3, 2.0)])
    both = metrics.roi_peak(dev(stack), index, fp, keep=k)
    assert both[0] == peaks and len(both) == 2 and both[1] != peaks


def test_roi_report_with_a_spacing_and_draws():
    fp64 = P.footprint(SPACING)
    lab = _regions()
    target, estimate = _pet(10), _pet(11, 2.5)
    draws = np.stack([_pet(12, 0.5), _pet(13, 1.0), _pet(14, 1.7)])
    keep = np.ones(SHAPE, dtype=np.uint8)
    keep[0] = keep[:, -1] = 0                                 # like the blend's zero-weight planes
    index = metrics.roi_index(dev(lab), keep=dev(keep))
    plain = metrics.roi_report(dev(estimate), dev(target), index, draws=dev(draws))
    rep = metrics.roi_report(dev(estimate), dev(target), index, draws=dev(draws), spacing=SPACING, keep=dev(keep))
    peaks = {}
    for name, vol in [("target", target), ("estimate", estimate)] + [("draw%d" % i, d) for i, d in enumerate(draws)]:
        mean, _, bound = P.sphere_mean(vol, fp64, keep)
        peaks[name] = P.region_peaks(mean, bound, lab, index.labels, keep)
    new_t = {"volume_ml", "tlg", "peak"}
    new_e = new_t | {"tlg_bias_rel", "peak_bias_rel", "draw_peaks", "peak_std"}
    for r, v in enumerate(index.labels):
        t, e = rep[v]["target"], rep[v]["estimate"]
        assert {k: x for k, x in t.items() if k not in new_t} == plain[v]["target"] and new_t <= set(t)
        assert {k: x for k, x in e.items() if k not in new_e} == plain[v]["estimate"] and new_e <= set(e)
        for block, vol, name in ((t, target, "target"), (e, estimate, "estimate")):
            want = P.figures(vol, lab, v, SPACING, keep)
            assert block["n"] == want["n"]
            assert block["volume_ml"] == pytest.approx(want["volume_ml"], rel=1e-6)
            assert block["tlg"] == pytest.approx(want["tlg"], rel=1e-6)
            assert abs(block["peak"] - peaks[name][r][0]) <= peaks[name][r][1]
        tp, ep = peaks["target"][r][0], peaks["estimate"][r][0]
        wt, we = P.figures(target, lab, v, SPACING, keep), P.figures(estimate, lab, v, SPACING, keep)
        assert e["tlg_bias_rel"] == pytest.approx((we["tlg"] - wt["tlg"]) / wt["tlg"], rel=1e-6)
        assert e["peak_bias_rel"] == pytest.approx((ep - tp) / tp, rel=1e-6)
        dp = [peaks["draw%d" % i][r] for i in range(3)]
        assert len(e["draw_peaks"]) == 3
        for got, (want, bound) in zip(e["draw_peaks"], dp):
            assert abs(got - want) <= bound
        assert e["peak_std"] == pytest.approx(float(np.std([p[0] for p in dp], ddof=1)), rel=1e-6)
        print("region %d: peak %.7g (target %.7g), bias %.6g, std over draws %.6g, %.4g ml, TLG %.6g"
              % (v, e["peak"], t["peak"], e["peak_bias_rel"], e["peak_std"], e["volume_ml"], e["tlg"]))
    # draws given as records need their peaks given too; another sphere volume gives other peaks
    recs = metrics.roi_moments(dev(draws), index)
    by_records = metrics.roi_report(dev(estimate), dev(target), index, draws=recs, spacing=SPACING, keep=dev(keep),
                                    draw_peaks=metrics.roi_peak(dev(draws), index, metrics.sphere_footprint(SPACING),
                                                                keep=dev(keep)))
    assert by_records == rep
    small = metrics.roi_report(dev(estimate), dev(target), index, spacing=SPACING, keep=dev(keep), volume_mm3=200.0)
    mean, _, bound = P.sphere_mean(estimate, P.footprint(SPACING, 200.0), keep)
    for r, (want, b) in enumerate(P.region_peaks(mean, bound, lab, index.labels, keep)):
        assert abs(small[index.labels[r]]["estimate"]["peak"] - want) <= b
    assert small[4]["estimate"]["peak"] != rep[4]["estimate"]["peak"]


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
FILE_SPACING = (3.27, 2.0, 1.5)                               # along the file's (D, H, W)
NEW_ROI = {"voxel_spacing", "peak_volume_mm3", "peak_taps"}
NEW_REGION = {"volume_ml", "tlg", "tlg_bias_rel", "peak", "peak_bias_rel", "draw_peaks", "peak_std"}


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra,draws,labelled", [
    ([], 0, True),
    (["--patch_overlap", "4", "--num_draws", "2", "--roi_threshold_frac", "0.4", "--roi_connectivity", "6"], 2, False),
], ids=["one-shot-labels", "sliding-draws-threshold"])
def test_script_writes_peak_volume_and_tlg(extra, draws, labelled, tmp_path):
    import metrics_ref
    target = metrics_ref.phantom((20, 40, 40), seed=4)                      # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = metrics_ref.noisy(target, 0.1, seed=4)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz")]
    common += extra
    if labelled:
        lab = np.zeros(target.shape, dtype=np.int32)
        lab[0:6, 2:9, 30:40] = 2                                            # reaches the planes the blend leaves at 0
        lab[8:14, 15:25, 10:22] = 5
        lab[10, 30, 30] = 9
        np.save(tmp_path / "lab.npy", lab)
        common += ["--roi_labels", str(tmp_path / "lab.npy")]
    mod = _script()
    path = mod.main(common + ["--save_dir", str(tmp_path / "mm"), "--voxel_spacing"] + [str(v) for v in FILE_SPACING])
    roi = json.load(open(tmp_path / "mm" / "metrics_pet.json"))["roi"]
    assert NEW_ROI <= set(roi) and roi["voxel_spacing"] == list(FILE_SPACING) and roi["peak_volume_mm3"] == 1000.0
    spacing = (FILE_SPACING[1], FILE_SPACING[2], FILE_SPACING[0])           # (H, W, Z), as the volumes are written
    fp = P.footprint(spacing)
    assert roi["peak_taps"] == int(fp.sum()) == 105

    out = np.load(path)
    arr = out["arr_0"]                                                       # (H, W, Z)
    hwz = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0))
    if not labelled:
        lab = np.load(tmp_path / "mm" / "roi_labels_pet.npz")["arr_0"]
    labels = hwz(lab)
    keep = np.zeros(arr.shape, dtype=np.uint8)                              # Hann weight 0: the outermost planes
    keep[1:-1, 1:-1, 1:-1] = 1
    values = [int(v) for v in np.unique(labels[keep != 0]) if v > 0]
    assert list(roi["regions"]) == [str(v) for v in values] and len(values) >= 3
    for name, vol in (("target", hwz(target)), ("input", hwz(low)), ("denoised", arr)):
        mean, _, bound = P.sphere_mean(vol, fp, keep)
        for v, (want, b) in zip(values, P.region_peaks(mean, bound, labels, values, keep)):
            block = roi["regions"][str(v)][name]
            fig = P.figures(vol, labels, v, spacing, keep)
            assert block["n"] == fig["n"]
            assert abs(block["peak"] - want) <= b, (name, v, block["peak"], want, b)
            assert block["volume_ml"] == pytest.approx(fig["volume_ml"], rel=1e-6)
            assert block["tlg"] == pytest.approx(fig["tlg"], rel=1e-6)
            assert ("peak_bias_rel" in block) == ("tlg_bias_rel" in block) == (name != "target")
            assert ("draw_peaks" in block) == ("peak_std" in block) == (name == "denoised" and bool(draws))
            if "draw_peaks" in block:
                assert len(block["draw_peaks"]) == draws
                assert block["peak_std"] == pytest.approx(float(np.std(block["draw_peaks"], ddof=1)), rel=1e-6)
    # the same command without the flag: none of the new keys, and the old ones with the same values
    assert mod.main(common + ["--save_dir", str(tmp_path / "plain")]) is not None
    plain = json.load(open(tmp_path / "plain" / "metrics_pet.json"))["roi"]
    assert not NEW_ROI & set(plain) and set(plain) == set(roi) - NEW_ROI
    for v, r in plain["regions"].items():
        for name in ("target", "input", "denoised"):
            assert not NEW_REGION & set(r[name])
            assert r[name] == {k: x for k, x in roi["regions"][v][name].items() if k not in NEW_REGION}
    assert open(tmp_path / "plain" / "denoised_pet.npz", "rb").read() == open(path, "rb").read()
