"""
CPU tier of the distance transform and the lesion boundary figures: the yardstick
(tests/edt_ref.py) against the all-pairs definition, the fp32 three-pass definition of include/ddpm3d.h against the
yardstick under its 5-rounding bound, every refusal of ddpm3d_distance_sq through the built library (it returns
before any launch), the Python functions' refusals, the script's flag checks, the condition the GPU tier's
edge-profile comparison rests on (no voxel of the yardstick within the bound of a shell edge), and the phantom's rows
for the README's table.  Nothing here touches a device.
"""

import numpy as np
import pytest

import edt_ref as R
from guided_diffusion import _hip, metrics

TINY = ((5, 6, 7), (1, 9, 4), (8, 1, 1), (3, 3, 11))
ALL_SPACINGS = ((1.0, 1.0, 1.0),) + R.SPACINGS


# ------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("spacing", ALL_SPACINGS[:3], ids=str)
@pytest.mark.parametrize("shape", TINY, ids=str)
def test_yardstick_is_the_all_pairs_minimum(shape, spacing):
    for k, density in enumerate((0.3, 0.8, 0.97)):
        mask = R.random_mask(shape, density, seed=10 * k + sum(shape))
        for invert in (False, True):
            want = R.brute(mask, spacing, invert)
            got = R.distance_sq(mask, spacing, invert)
            # both are fp64 sums of the same three squares, at most summed in another order
            assert np.allclose(got, want, rtol=4 * 2.0 ** -52, atol=0.0)
            assert np.array_equal(got == 0, R.foreground(mask, invert) == 0)


def test_yardstick_without_background_and_without_foreground():
    ones = np.ones((3, 4, 5), dtype=np.uint8)
    assert np.isinf(R.distance_sq(ones, (1, 2, 3))).all() and np.isinf(R.brute(ones, (1, 2, 3))).all()
    assert not R.distance_sq(ones, (1, 2, 3), invert=True).any() and not R.brute(0 * ones, (1, 2, 3)).any()


def test_yardstick_is_an_exact_integer_at_unit_spacing():
    mask = R.random_mask((9, 10, 11), 0.95, seed=3)
    got = R.distance_sq(mask, (1, 1, 1))
    assert np.array_equal(got, np.rint(got)) and got.max() >= 4


# ------------------------------------------------------------------------------------------ the definition
def test_the_three_fp32_passes_are_exact_at_unit_spacing():
    mask = R.random_mask((7, 9, 12), 0.9, seed=5)
    assert np.array_equal(R.emulate(mask, (1, 1, 1)).astype(np.float64), R.distance_sq(mask, (1, 1, 1)))


@pytest.mark.parametrize("spacing", R.SPACINGS, ids=str)
def test_the_three_fp32_passes_hold_the_bound(spacing, capsys):
    worst = 0.0
    for k, density in enumerate((0.5, 0.9, 0.99)):
        mask = R.random_mask((9, 11, 17), density, seed=20 + k)
        worst = max(worst, R.share_of_bound(R.emulate(mask, spacing), R.distance_sq(mask, spacing)))
    with capsys.disabled():
        print("\nfp32 passes at %s: %.3f of the bound" % (spacing, worst))
    assert worst <= 1.0


def test_bound_constants():
    assert R.BOUND == (1 + 2.0 ** -24) ** 5 - 1 and 5 * 2.0 ** -24 < R.BOUND < 5.000002 * 2.0 ** -24
    assert _hip.EDT_MAX_EXTENT >= 1024 and _hip.EDT_COLUMNS * _hip.EDT_MAX_EXTENT * 4 <= 64 * 1024


# ------------------------------------------------------------------------------------------ the entry's refusals
def test_distance_sq_refusals_return_before_any_launch():
    """no device is present here: a call that got as far as a launch would fail in another way"""
    lib = _hip.load()
    mask, out = 1 << 20, 1 << 32                             # never dereferenced by a refused call
    top = _hip.EDT_MAX_EXTENT

    def call(mask=mask, K=1, D=3, H=7, W=13, invert=0, s=(3.27, 2.0, 2.0), out=out):
        return lib.ddpm3d_distance_sq(mask, K, D, H, W, invert, s[0], s[1], s[2], out, None)

    nan, inf = float("nan"), float("inf")
    bad = [
        dict(mask=None), dict(out=None), dict(K=0), dict(K=-1), dict(D=0), dict(H=0), dict(W=0), dict(W=-3),
        dict(D=top + 1), dict(H=top + 1), dict(W=top + 1), dict(invert=2), dict(invert=-1),
        dict(s=(0.0, 2.0, 2.0)), dict(s=(3.0, -2.0, 2.0)), dict(s=(3.0, 2.0, nan)), dict(s=(inf, 2.0, 2.0)),
        dict(s=(1e39, 2.0, 2.0)), dict(s=(3.0, 1e-46, 2.0)),        # inf and 0 once rounded to fp32
        dict(K=1 << 21, D=top, H=1, W=1),                            # K * D * H rows: 2^31
        dict(K=1 << 27, D=1, H=1, W=top),                            # K * D * ceil(W / 16) workgroups: 2^33
        dict(out=mask), dict(out=mask + 3 * 7 * 13 - 1), dict(out=mask - 4 * 3 * 7 * 13 + 1),
    ]
    for kw in bad:
        assert call(**kw) == _hip.E_INVAL, kw
        assert lib.ddpm3d_last_error().decode().startswith("distance_sq:"), kw


def test_python_refusals_come_before_the_library():
    import torch
    host = torch.zeros((3, 4, 5), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.distance_sq(host, (1, 1, 1))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.surface(host)
    with pytest.raises(ValueError, match="three positive finite"):
        metrics.distance_sq(host, (1, 1))
    with pytest.raises(ValueError, match="three positive finite"):
        metrics.distance_sq(host, (1, 0, 1))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.boundary(host.int(), host.int(), (1, 1, 1))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.edge_profile({"x": host.float()}, host.int(), (1, 1, 1), 2.0)


def test_percentile_positions_are_numpys():
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 19, 20, 21, 22, 40, 41, 101, 1000):
        v = np.sort(rng.random(n))
        lo, hi, t = metrics._percentile_at(n)
        assert metrics._lerp(float(v[lo]), float(v[hi]), t) == float(np.percentile(v, 95, method="linear")), n


# ------------------------------------------------------------------------------------------ the consumers' yardstick
def test_surface_of_a_box_is_its_shell():
    m = np.zeros((6, 7, 8), dtype=bool)
    m[1:5, 0:7, 2:7] = True                                 # touches the volume's faces along H
    s = R.surface(m)
    inner = np.zeros_like(m)
    inner[2:4, 1:6, 3:6] = True
    assert np.array_equal(s, m & ~inner)


def test_boundary_yardstick_on_the_blobs():
    t, e, _, _ = R.blobs()
    spacing = (3.0, 2.0, 2.0)
    fig, sets = R.boundary(t, e, spacing)
    assert fig["n_surface_target"] == len(sets["t"]) and fig["n_surface_estimate"] == len(sets["e"])
    assert 0.0 < fig["dice"] < 1.0 and fig["jaccard"] == pytest.approx(fig["dice"] / (2.0 - fig["dice"]))
    # the missed lesion's surface is far from the only estimate component; the shifted one's is within a voxel
    assert fig["regions"][1]["surface_max_mm"] == fig["hd_mm"] > 10.0
    assert 0.0 < fig["regions"][2]["surface_max_mm"] <= 2.0
    assert fig["hd95_mm"] <= fig["hd_mm"] and fig["assd_mm"] < fig["hd_mm"]
    same, _ = R.boundary(t, t, spacing)
    assert same["dice"] == 1.0 and same["hd_mm"] == 0.0 and same["assd_mm"] == 0.0
    none, _ = R.boundary(t, 0 * t, spacing)
    assert none["dice"] == 0.0 and none["hd_mm"] is None and none["regions"][1]["surface_mean_mm"] is None


EDGE_CASE = dict(spacing=(2.0, 2.0, 2.0), width=2.5, inside=3, outside=3)
EDGE_CASE_KW = {k: EDGE_CASE[k] for k in ("spacing", "width", "inside", "outside")}


def test_no_voxel_of_the_yardstick_lies_within_the_bound_of_a_shell_edge():
    """squared distances at 2 mm are 4 k, k an integer; the squared edges (2.5 j)^2 are 6.25, 25 and 56.25, none a
    multiple of 4, so a squared distance stays at least 0.25 mm^2 from every edge, far above the bound: the GPU tier
    may compare the shells' counts for equality.  The cap is zero voxels within the bound."""
    t, _, _, _ = R.blobs()
    number, gap = R.shells(t, EDGE_CASE["spacing"], EDGE_CASE["width"], EDGE_CASE["inside"], EDGE_CASE["outside"])
    within = gap <= R.BOUND_MM
    assert not within and gap > 1e-3
    assert set(np.unique(number)) == set(range(0, 7))       # every shell holds voxels


def test_edge_profile_yardstick_shows_the_step():
    t, _, vol, _ = R.blobs()
    prof = R.edge_profile({"target": vol}, t, **EDGE_CASE_KW)
    assert [r["distance_mm"] for r in prof["rows"]] == [-6.25, -3.75, -1.25, 1.25, 3.75, 6.25]
    assert [r["mean"]["target"] for r in prof["rows"]] == [4.0] * 3 + [1.0] * 3
    keep = np.ones(t.shape, dtype=np.uint8)
    keep[:, :, :20] = 0
    kept = R.edge_profile({"target": vol}, t, keep=keep, **EDGE_CASE_KW)
    assert all(a["n"] > b["n"] for a, b in zip(prof["rows"], kept["rows"]))


def test_phantom_rows_for_the_readme(capsys):
    """clean, noisy and Gaussian-filtered (sigma = 1 voxel) 24 x 40 x 40 phantom at (3.27, 2, 2) mm, every volume
    segmented at 0.4 of the clean maximum, 26-connectivity, at least 5 voxels: the README's table"""
    import segment_ref
    clean, low, smooth = R.phantom_rows()
    spacing = (3.27, 2.0, 2.0)
    threshold = float(np.float32(0.4 * float(clean.max())))
    target, n = segment_ref.segment(clean, threshold, 26, 5)
    rows = {}
    for name, vol in (("clean", clean), ("noisy", low), ("gaussian", smooth)):
        est, _ = segment_ref.segment(vol, threshold, 26, 5)
        rows[name] = R.boundary(target, est, spacing)[0]
    prof = R.edge_profile({"clean": clean, "noisy": low, "gaussian": smooth}, target, spacing, 2.5)
    with capsys.disabled():
        print("\n%d lesions, %d surface voxels" % (n, rows["clean"]["n_surface_target"]))
        for name, f in rows.items():
            print("%-9s Dice %.4f  Jaccard %.4f  HD %.3f mm  HD95 %.3f mm  ASSD %.4f mm  surface %d"
                  % (name, f["dice"], f["jaccard"], f["hd_mm"], f["hd95_mm"], f["assd_mm"], f["n_surface_estimate"]))
        for r in prof["rows"]:
            print("%+6.2f mm  n %5d  clean %.4f  noisy %.4f  gaussian %.4f"
                  % (r["distance_mm"], r["n"], r["mean"]["clean"], r["mean"]["noisy"], r["mean"]["gaussian"]))
    assert n >= 3
    assert rows["clean"]["dice"] == 1.0 and rows["clean"]["hd_mm"] == 0.0 and rows["clean"]["assd_mm"] == 0.0
    assert rows["noisy"]["dice"] < rows["gaussian"]["dice"] < 1.0       # the filter mends the ragged edge
    assert rows["gaussian"]["assd_mm"] < rows["noisy"]["assd_mm"]
    means = [r["mean"] for r in prof["rows"]]
    # the lesions are hotter than what surrounds them: the clean profile falls outward; the filter spills activity out
    # of them, so it is below the clean one in every inside shell and its step from the innermost to the outermost
    # shell is smaller
    assert all(a["clean"] > b["clean"] for a, b in zip(means, means[1:]))
    assert all(m["gaussian"] < m["clean"] for m in means[:3])
    assert means[0]["gaussian"] - means[-1]["gaussian"] < means[0]["clean"] - means[-1]["clean"]


# ------------------------------------------------------------------------------------------ the script's flags
def _script():
    import importlib.util
    import os
    from conftest import PKG
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


def _files(tmp_path, shape=(12, 16, 24)):
    np.savez(tmp_path / "low.npz", np.zeros(shape, dtype=np.float32))
    np.savez(tmp_path / "full.npz", np.ones(shape, dtype=np.float32))
    labels = np.zeros(shape, dtype=np.int32)
    labels[2:5, 2:5, 2:5] = 1
    labels[6:9, 8:12, 8:12] = 2
    np.savez(tmp_path / "labels.npz", labels)
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]


def _flags(tmp_path):
    mm = ["--voxel_spacing", "3.27", "2", "1.5"]
    target = ["--target_samples", str(tmp_path / "full.npz")]
    return mm, target, ["--roi_threshold", "0.5"], ["--roi_labels", str(tmp_path / "labels.npz")]


SCRIPT_CASES = {
    "boundary_no_threshold": (lambda mm, t, thr, lab: ["--roi_boundary", "True"] + mm + t + lab,
                              "--roi_boundary needs --roi_threshold or --roi_threshold_frac", (12, 16, 24)),
    "boundary_no_spacing": (lambda mm, t, thr, lab: ["--roi_boundary", "True"] + t + thr,
                            "--roi_boundary needs --voxel_spacing", (12, 16, 24)),
    "boundary_no_target": (lambda mm, t, thr, lab: ["--roi_boundary", "True"] + mm + thr,
                           "needs --target_samples", (12, 16, 24)),
    "profile_no_target": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "2"] + mm,
                          "--roi_edge_profile_mm needs --target_samples", (12, 16, 24)),
    "profile_no_spacing": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "2"] + t + lab,
                           "--roi_edge_profile_mm needs --voxel_spacing", (12, 16, 24)),
    "profile_no_regions": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "2"] + mm + t,
                           "--roi_edge_profile_mm needs regions", (12, 16, 24)),
    "profile_zero": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "0"] + mm + t + lab,
                     "must be a positive finite width", (12, 16, 24)),
    "profile_nan": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "nan"] + mm + t + lab,
                    "must be a positive finite width", (12, 16, 24)),
    "profile_inf": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "inf"] + mm + t + lab,
                    "must be a positive finite width", (12, 16, 24)),
    "profile_thin": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "1.4"] + mm + t + lab,
                     "is below the smallest voxel spacing 1.5 mm", (12, 16, 24)),
    "boundary_long": (lambda mm, t, thr, lab: ["--roi_boundary", "True"] + mm + t + thr,
                      "the distance transform takes extents up to %d" % _hip.EDT_MAX_EXTENT,
                      (11, 11, _hip.EDT_MAX_EXTENT + 1)),
    "profile_long": (lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "2"] + mm + t + thr,
                     "the distance transform takes extents up to %d" % _hip.EDT_MAX_EXTENT,
                     (_hip.EDT_MAX_EXTENT + 1, 11, 11)),
}


@pytest.mark.parametrize("case", sorted(SCRIPT_CASES))
def test_script_refuses_bad_boundary_flags_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, text, shape = SCRIPT_CASES[case]
    with pytest.raises(SystemExit) as e:
        mod.main(_files(tmp_path, shape) + extra(*_flags(tmp_path)))
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err[err.rindex("error:"):]


@pytest.mark.parametrize("extra", [
    lambda mm, t, thr, lab: ["--roi_boundary", "True"] + mm + t + thr,
    lambda mm, t, thr, lab: ["--roi_edge_profile_mm", "1.5"] + mm + t + lab + ["--roi_background", "2"],
    lambda mm, t, thr, lab: ["--roi_boundary", "True", "--roi_edge_profile_mm", "4", "--joint_patches", "True",
                             "--num_draws", "2"] + mm + t + thr,
], ids=["boundary", "profile", "both-joint-draws"])
def test_script_accepts_good_boundary_flags(extra, tmp_path, monkeypatch):
    mod = _script()
    _no_device(mod, monkeypatch)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path) + extra(*_flags(tmp_path)))


def test_script_defaults_are_off():
    args = _script().create_argparser().parse_args([])
    assert args.roi_boundary is False and args.roi_edge_profile_mm is None
