"""
CPU tier of the radial spectra and the Fourier shell correlation: the host side of
metrics.spectrum_plan (tables, windows, q tables, shell numbers, refusals) against numpy.fft and the restatement of
tests/spectrum_ref.py, metrics.spectrum_figures on constructed records, the Gaussian's known power ratio, and the
24 x 40 x 40 phantom's rows for the README's table.  Nothing here touches a device.
"""

import math

import numpy as np
import pytest

import spectrum_ref as R
from guided_diffusion import _hip, metrics

ISO = (2.0, 2.0, 2.0)
ANISO = (3.27, 2.0, 1.5)


def _multiply_out(plan, v):
    """the three passes W, H, D with the plan's fp32 tables widened to fp64: what the kernel evaluates, exactly"""
    c, s = [t.astype(np.float64) for t in plan.cos], [t.astype(np.float64) for t in plan.sin]
    x = np.einsum("kx,dhx->dhk", c[2] + 1j * s[2], v)
    x = np.einsum("kh,dhw->dkw", c[1] + 1j * s[1], x)
    return np.einsum("kd,dhw->khw", c[0] + 1j * s[0], x)


@pytest.mark.parametrize("window", ["hann", "none"])
@pytest.mark.parametrize("shape", [(5, 6, 7), (8, 9, 10)])
def test_the_tables_multiplied_out_are_rfftn(shape, window):
    plan = metrics.spectrum_plan(shape, ISO, window=window)
    v = np.random.default_rng(1).normal(size=shape)
    want = np.fft.rfftn(R.weight(window, shape) * v)
    got = _multiply_out(plan, v)
    scale = np.abs(want).max()
    # the tables are rounded to fp32 once: 2^-24 relative per entry, three passes
    assert np.abs(got - want).max() <= 3 * 2.0 ** -24 * np.abs(R.weight(window, shape) * v).sum()
    c, s = zip(*[metrics._dft_tables(n, rows, w) for n, rows, w in zip(shape, plan.rows, plan.windows)])
    for a, (n, rows) in enumerate(zip(shape, plan.rows)):              # before that rounding: 1e-12
        assert plan.cos[a].dtype == np.float32 and plan.cos[a].shape == (rows, n) and c[a].dtype == np.float64
        assert np.array_equal(plan.cos[a], c[a].astype(np.float32))    # rounded once
        assert np.array_equal(plan.sin[a], s[a].astype(np.float32))
        rc, rs = R.tables(n, rows, R.window(window, n))
        assert np.abs(c[a] - rc).max() <= 1e-15 and np.abs(s[a] - rs).max() <= 1e-15
        assert np.allclose(plan.windows[a], R.window(window, n), rtol=0, atol=1e-15)
    x = np.einsum("kx,dhx->dhk", c[2] + 1j * s[2], v)
    x = np.einsum("kh,dhw->dkw", c[1] + 1j * s[1], x)
    x = np.einsum("kd,dhw->khw", c[0] + 1j * s[0], x)
    assert np.abs(x - want).max() <= 1e-12 * max(scale, 1.0)
    if window == "hann":
        assert all((w > 0).all() and np.allclose(w, w[::-1]) for w in plan.windows)


@pytest.mark.parametrize("spacing", [ISO, ANISO])
@pytest.mark.parametrize("shape", [(5, 6, 7), (8, 9, 10), (24, 40, 40)])
def test_shell_tables(shape, spacing):
    plan = metrics.spectrum_plan(shape, spacing)
    width = R.default_width(shape, spacing)
    assert plan.shell_width == width
    half = plan.shell_numbers()
    assert half.shape == (shape[0], shape[1], shape[2] // 2 + 1)
    assert np.array_equal(half, R.shell_numbers(shape, spacing, half=True))
    full = R.shell_numbers(shape, spacing)
    assert plan.shells == full.max() + 1 == half.max() + 1
    # the count per shell of the full spectrum, from the half spectrum's twin weights: it sums to D H W
    kw = np.arange(shape[2] // 2 + 1)
    twin = np.where((kw > 0) & (2 * kw != shape[2]), 2, 1)
    counts = np.bincount(half.reshape(-1), weights=np.broadcast_to(twin, half.shape).reshape(-1), minlength=plan.shells)
    assert counts.sum() == np.prod(shape)
    assert np.array_equal(counts, np.bincount(full.reshape(-1), minlength=plan.shells))
    assert np.allclose(plan.frequency, (np.arange(plan.shells) + 0.5) * width, rtol=1e-15)
    nyq = min(1 / (2 * s) for s in spacing)
    assert plan.n_reported == sum((s + 1) * width <= nyq for s in range(plan.shells))
    assert 1 <= plan.n_reported <= plan.shells


def test_the_integer_shell_rule_on_exact_squares():
    r2 = np.array([0.0, 0.999999999, 1.0, 3.9999999999999996, 4.0, 4.000000000000001, 8.99, 9.0, 4095.0 ** 2,
                   np.nextafter(4095.0 ** 2, 0)])
    want = [0, 0, 1, 1, 2, 2, 2, 3, 4095, 4094]
    assert metrics._shell_of(r2, np).tolist() == want and R.shell_of(r2).tolist() == want
    # an 8^3 grid at unit spacing: q = k~^2 exactly, so (2, 0, 0) has r2 = 4.0 and lies in shell 2, (1, 1, 1) in 1
    plan = metrics.spectrum_plan((8, 8, 8), (1, 1, 1))
    sh = plan.shell_numbers()
    assert plan.shell_width == 1 / 8 and sh[2, 0, 0] == 2 and sh[0, 6, 0] == 2 and sh[1, 1, 1] == 1
    assert sh[4, 4, 4] == 6 and plan.shells == 7 and sh[0, 0, 3] == 3 and sh[7, 0, 0] == 1


def _agree(a, b, rel=1e-12):
    """two figure dicts: the same keys and Nones, numbers within rel (the two normalise by differently ordered sums)"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b)
        for k in a:
            _agree(a[k], b[k], rel)
    elif isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _agree(x, y, rel)
    elif a is None or isinstance(a, bool):
        assert a is b
    else:
        assert b is not None and a == pytest.approx(b, rel=rel, abs=0)


def _records(fsc, ratio, plan):
    rec = np.zeros((plan.shells, _hip.SP_REC))
    rec[:, _hip.SP_N] = 10
    rec[:, _hip.SP_SUM_YY] = 4.0
    rec[:len(ratio), _hip.SP_SUM_XX] = 4.0 * np.asarray(ratio)
    rec[:len(fsc), _hip.SP_SUM_XY] = np.asarray(fsc) * np.sqrt(rec[:len(fsc), _hip.SP_SUM_XX] * 4.0)
    rec[:, _hip.SP_SUM_EE] = rec[:, _hip.SP_SUM_XX] + 4.0 - 2 * rec[:, _hip.SP_SUM_XY]
    return rec


def test_figures_on_constructed_records():
    shape = (24, 40, 40)
    plan = metrics.spectrum_plan(shape, ISO)
    n = plan.n_reported
    assert n >= 8
    same = _records(np.ones(plan.shells), np.ones(plan.shells), plan)
    fig = metrics.spectrum_figures(same, plan)
    assert fig["fsc"] == [1.0] * n and fig["ratio"] == [1.0] * n and fig["error_rel"] == [0.0] * n
    assert fig["fsc_resolution_mm"] == {"0.5": None, "0.143": None, "to_nyquist": True}
    assert fig["ratio_half_mm"] is None and fig["n"] == [10] * n
    assert fig["frequency"] == [(s + 0.5) * plan.shell_width for s in range(n)]
    assert fig["power"] == [4.0 / (plan.voxels * plan.weight_sq)] * n == fig["power_target"]
    _agree(fig, R.figures(same, shape, ISO, "hann"))
    # a curve through 0.8, 0.6, 0.4, 0.2, 0.1: 0.5 is crossed half way between the centres of shells 2 and 3, 1/7
    # between shells 4 and 5
    fsc = [1.0, 0.8, 0.6, 0.4, 0.2, 0.1] + [0.05] * (plan.shells - 6)
    ratio = [1.0, 0.9, 0.5, 0.3, 0.2] + [0.1] * (plan.shells - 5)
    fig = metrics.spectrum_figures(_records(fsc, ratio, plan), plan)
    f = plan.frequency
    assert fig["fsc_resolution_mm"]["0.5"] == pytest.approx(1 / (0.5 * (f[2] + f[3])), rel=1e-12)
    assert fig["fsc_resolution_mm"]["0.143"] == pytest.approx(1 / (f[4] + (0.2 - 1 / 7) / 0.1 * (f[5] - f[4])), rel=1e-12)
    assert fig["fsc_resolution_mm"]["to_nyquist"] is False
    assert fig["ratio_half_mm"] == pytest.approx(1 / (0.5 * (f[3] + f[4])), rel=1e-12)
    _agree(fig, R.figures(_records(fsc, ratio, plan), shape, ISO, "hann"))
    # a zero denominator and a non-finite sum give None, and K records give K dicts
    hole = _records(fsc, ratio, plan)
    hole[3, _hip.SP_SUM_YY] = 0.0
    hole[5, _hip.SP_SUM_XX] = np.nan
    two = metrics.spectrum_figures(np.stack([hole, same]), plan)
    assert isinstance(two, list) and two[1] == metrics.spectrum_figures(same, plan)
    assert two[0]["fsc"][3] is None and two[0]["ratio"][3] is None and two[0]["error_rel"][3] is None
    assert two[0]["fsc"][5] is None and two[0]["power"][5] is None and two[0]["ratio"][5] is None
    assert two[0]["fsc_resolution_mm"] == {"0.5": None, "0.143": None, "to_nyquist": False}
    # below the threshold from the first shell on: its centre
    low = metrics.spectrum_figures(_records([1.0] + [0.3] * (plan.shells - 1), np.ones(plan.shells), plan), plan)
    assert low["fsc_resolution_mm"]["0.5"] == 1 / f[1] and low["fsc_resolution_mm"]["0.143"] is None
    with pytest.raises(ValueError):
        metrics.spectrum_figures(same[:-1], plan)


def test_a_periodic_gaussian_has_its_known_power_ratio():
    from scipy.ndimage import gaussian_filter
    shape, spacing, sigma = (24, 40, 40), (2.0, 2.0, 2.0), 1.0
    noise = np.random.default_rng(3).normal(size=shape)
    smooth = gaussian_filter(noise, sigma, mode="wrap", truncate=8.0)
    sh = R.shell_numbers(shape, spacing)
    S = int(sh.max()) + 1
    rec = R.records(np.fft.fftn(smooth), np.fft.fftn(noise), sh, S)
    plan = metrics.spectrum_plan(shape, spacing, window="none")
    assert plan.shells == S
    fig = metrics.spectrum_figures(rec, plan)
    # Per coefficient |G|^2 = exp(-4 pi^2 sigma^2 f^2), f in cycles per voxel, for the continuous Gaussian.  The
    # filter samples it at the voxels, which adds its aliases: per axis G(f) = sum_m exp(-2 pi^2 sigma^2 (f + m)^2) /
    # sum_m exp(-2 pi^2 sigma^2 m^2) (Poisson summation; the truncation at 8 sigma is e^-32).  So the sampled curve is
    # the continuous one times (1 + eps), 0 <= eps, and a shell's |Y|^2-weighted ratio lies between the weighted mean
    # of the continuous curve and (1 + the shell's largest eps) times it.
    m = np.arange(-4, 5)
    axes = [np.fft.fftfreq(n) for n in shape]
    alias = [np.exp(-2 * np.pi ** 2 * sigma ** 2 * (f[:, None] + m[None, :]) ** 2).sum(axis=1)
             / np.exp(-2 * np.pi ** 2 * sigma ** 2 * m ** 2).sum() for f in axes]
    sampled = (alias[0][:, None, None] * alias[1][None, :, None] * alias[2][None, None, :]) ** 2
    f2 = axes[0][:, None, None] ** 2 + axes[1][None, :, None] ** 2 + axes[2][None, None, :] ** 2
    curve = np.exp(-4 * np.pi ** 2 * sigma ** 2 * f2)
    eps = sampled / curve - 1
    assert eps.min() > -1e-8
    yy = np.abs(np.fft.fftn(noise)) ** 2
    for s in range(plan.n_reported):
        mean = (curve * yy)[sh == s].sum() / yy[sh == s].sum()
        assert mean * (1 - 1e-8) <= fig["ratio"][s] <= mean * (1 + eps[sh == s].max()) * (1 + 1e-8), s
        assert fig["ratio"][s] == pytest.approx((sampled * yy)[sh == s].sum() / yy[sh == s].sum(), rel=1e-8), s
        # and against the plain shell mean: white noise weights a shell's n coefficients evenly but for the scatter of
        # |Y|^2 (exponential, relative std 1, twins pair up: n / 2 independent ones); six sigma of it
        n = (sh == s).sum()
        plain = curve[sh == s].mean()
        spread = curve[sh == s].std() / plain
        assert abs(mean / plain - 1) <= 6 * spread * math.sqrt(2.0 / n) + 1e-12, s
    assert fig["ratio_half_mm"] is not None
    # amplitude 1/2 at f = sqrt(ln 4) / (2 pi sigma) cycles per voxel
    want_mm = spacing[0] / (math.sqrt(math.log(4.0)) / (2 * math.pi * sigma))
    assert fig["ratio_half_mm"] == pytest.approx(want_mm, rel=0.1)


@pytest.mark.parametrize("kwargs, text", [
    (dict(shape=(5, 6, 7), spacing=(1, 1)), "three positive finite"),
    (dict(shape=(5, 6, 7), spacing=(1, 0, 1)), "three positive finite"),
    (dict(shape=(5, 6, 7), spacing=(1, float("nan"), 1)), "three positive finite"),
    (dict(shape=(5, 6, 7), spacing=(1, float("inf"), 1)), "three positive finite"),
    (dict(shape=(5, 6, 7), spacing=(1, -2, 1)), "three positive finite"),
    (dict(shape=(5, 6, 7), spacing=None), "three positive finite"),
    (dict(shape=(1, 6, 7), spacing=ISO), "2..2048"),
    (dict(shape=(5, 2049, 7), spacing=ISO), "2..2048"),
    (dict(shape=(5, 6), spacing=ISO), "2..2048"),
    (dict(shape=(5, 6, 7), spacing=ISO, window="hamming"), "window"),
    (dict(shape=(5, 6, 7), spacing=ISO, window=None), "window"),
    (dict(shape=(5, 6, 7), spacing=ISO, shell_width=0.0), "shell width"),
    (dict(shape=(5, 6, 7), spacing=ISO, shell_width=float("nan")), "shell width"),
    (dict(shape=(5, 6, 7), spacing=ISO, shell_width=1e-5), "shells"),
    (dict(shape=(5, 6, 7), spacing=ISO, shell_width=1e-12), "shells"),
])
def test_plan_refusals(kwargs, text):
    with pytest.raises(ValueError, match=text):
        metrics.spectrum_plan(**kwargs)


def test_the_widest_plans_pass():
    assert metrics.spectrum_plan((2, 2, 2), ISO).shells == 2
    plan = metrics.spectrum_plan((8, 8, 8), (1, 1, 1), shell_width=0.8661 / 4096)    # sqrt(3) / 2 = 0.86603
    assert plan.shells == 4096                                                      # the cap itself
    with pytest.raises(ValueError, match="4097 shells"):
        metrics.spectrum_plan((8, 8, 8), (1, 1, 1), shell_width=0.866 / 4096)
    assert metrics.spectrum_plan((5, 6, 7), ISO, shell_width=10.0).shells == 1


def test_phantom_rows_for_the_readme(capsys):
    """clean, noisy and Gaussian-filtered (sigma = 1 voxel) 24 x 40 x 40 phantom at 2 mm: the README's table"""
    clean, low, smooth = R.phantom_rows()
    spacing = (2.0, 2.0, 2.0)
    plan = metrics.spectrum_plan(clean.shape, spacing)
    rec = R.shell_records(np.stack([clean, low, smooth]), clean, spacing, "hann")
    figs = metrics.spectrum_figures(rec, plan)
    with capsys.disabled():
        print()
        for name, f in zip(("clean", "noisy", "gaussian"), figs):
            print("%-9s FSC 0.5 at %s mm, FSC 1/7 at %s mm, ratio 1/2 at %s mm; ratio at %.3f c/mm: %.3f" % (
                name, f["fsc_resolution_mm"]["0.5"], f["fsc_resolution_mm"]["0.143"], f["ratio_half_mm"],
                f["frequency"][-1], f["ratio"][-1]))
    assert figs[0]["fsc"] == pytest.approx([1.0] * plan.n_reported, abs=1e-12)
    assert figs[0]["fsc_resolution_mm"]["to_nyquist"] is True and figs[0]["ratio_half_mm"] is None
    assert figs[1]["ratio"][-1] > 2.0                    # noise raises power where the target has little
    assert figs[2]["ratio"][-1] < figs[1]["ratio"][-1] * 0.05   # and the Gaussian takes it away again
    assert figs[2]["fsc"][-1] < figs[2]["fsc"][1]


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
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]


SPEC, MM = ["--spectrum", "True"], ["--voxel_spacing", "3.27", "2", "1.5"]
CASES = {
    "no_target": (SPEC + MM, "--spectrum needs --target_samples", (12, 16, 24)),
    "no_spacing": (SPEC, "--spectrum needs --voxel_spacing", (12, 16, 24)),
    "window": (SPEC + MM + ["--spectrum_window", "hamming"], "--spectrum_window must be one of hann, none", (12, 16, 24)),
    "spacing_two": (SPEC + ["--voxel_spacing", "2", "2"], "three numbers", (12, 16, 24)),
    "spacing_zero": (SPEC + ["--voxel_spacing", "2", "0", "2"], "positive finite", (12, 16, 24)),
    "box_above_2048": (SPEC + MM, "each must be in 2..2048", (11, 11, 2051)),
    "whole_above_2048": (SPEC + MM + ["--joint_patches", "True"], "each must be in 2..2048", (11, 11, 2049)),
    "too_many_draws": (SPEC + MM + ["--num_draws", "62", "--baseline_gaussian_fwhm", "5"], "one launch of at most 64",
                       (12, 16, 24)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_script_refuses_bad_spectrum_flags_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, text, shape = CASES[case]
    argv = _files(tmp_path, shape) + extra
    if case != "no_target":
        argv += ["--target_samples", str(tmp_path / "full.npz")]
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err[err.rindex("error:"):]


@pytest.mark.parametrize("flags, shape", [(SPEC + MM, (12, 16, 24)), (SPEC + MM + ["--spectrum_window", "none"], (12, 16, 24)),
                                          (SPEC + MM, (11, 11, 2050)),
                                          (SPEC + MM + ["--joint_patches", "True"], (11, 11, 2048)),
                                          (SPEC + MM + ["--num_draws", "61", "--baseline_gaussian_fwhm", "5"],
                                           (12, 16, 24))],
                         ids=["plain", "none", "box-2048", "joint-2048", "most-draws"])
def test_script_accepts_good_spectrum_flags_before_it_builds_the_model(flags, shape, tmp_path, monkeypatch):
    """no regions are needed: the spacing serves the spectrum; the checks above are the refusals' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path, shape) + ["--target_samples", str(tmp_path / "full.npz")] + flags)


def test_script_default_is_no_spectrum_and_the_box_follows_the_path():
    mod = _script()
    parser = mod.create_argparser()
    args = parser.parse_args([])
    assert args.spectrum is False and args.spectrum_window == "hann" and mod._check_spectrum(None, args) is None
    assert mod._spectrum_box(args, (24, 40, 40)) == ([1, 1, 1], [23, 39, 39])
    args = parser.parse_args(["--joint_patches", "True"])
    assert mod._spectrum_box(args, (24, 40, 40)) == ([0, 0, 0], [24, 40, 40])
