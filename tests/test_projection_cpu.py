"""
CPU tier of the rotating maximum-intensity and ray-sum projections: metrics.projection_plan's
defaults, tables and refusals, the properties of the yardstick (tests/projection_ref.py), the refusals of
ddpm3d_project_table_fill and ddpm3d_project through the built library (both return before any launch), the script's
--mip_angles checks, and the condition the GPU tier rests on: the yardstick alone flags at most 1 % of the outputs of
every shared case ambiguous.  Nothing here touches a device.
"""

import ctypes
import math

import numpy as np
import pytest

import projection_cases as PC
import projection_ref as R
from guided_diffusion import _hip, metrics


def _plan(case):
    return metrics.projection_plan(case["shape"], case["spacing"], PC.angles_of(case), **case["plan"])


# ------------------------------------------------------------------------------------------ the plan
def test_plan_defaults():
    plan = metrics.projection_plan((3, 7, 13), (3.0, 2.5, 2.0), [0, 45])
    assert plan.pitch == plan.step == 2.0
    want = math.ceil(math.hypot(7 * 2.5, 13 * 2.0) / 2.0)
    assert plan.bins == plan.samples == want == metrics.projection_default_bins((3, 7, 13), (3.0, 2.5, 2.0))
    assert plan.table.angles == 2 and plan.table.bins == want and plan.table.samples == want
    assert plan.table.step == 2.0 and plan.coef.shape == (2, 6) and plan.coef.dtype == np.float32
    # the slice's corners lie inside the detector and the ray at every angle
    half = 0.5 * want * 2.0
    assert half >= 0.5 * math.hypot(7 * 2.5, 13 * 2.0)
    plan = metrics.projection_plan((3, 7, 13), (3.0, 2.5, 2.0), [10.0], pitch=1.0, samples=5)
    assert plan.pitch == 1.0 and plan.step == 2.0 and plan.samples == 5
    assert plan.bins == math.ceil(math.hypot(17.5, 26.0) / 1.0)


def test_tables_are_exact_at_multiples_of_90_degrees():
    H, W, s1, s2, p, U, d, Rn = 7, 13, 2.5, 2.0, 2.0, 18, 1.0, 19
    plan = metrics.projection_plan((3, H, W), (3.0, s1, s2), [0, 90, 180, 270, 360, -90, 450], pitch=p, bins=U,
                                   step=d, samples=Rn)
    mu, mj, f = 0.5 * (U - 1), 0.5 * (Rn - 1), np.float32
    rows = {
        0: (0.5 * (H - 1) - mj * d / s1, 0.0, d / s1, 0.5 * (W - 1) - mu * p / s2, p / s2, 0.0),
        90: (0.5 * (H - 1) - mu * p / s1, p / s1, 0.0, 0.5 * (W - 1) + mj * d / s2, 0.0, -d / s2),
        180: (0.5 * (H - 1) + mj * d / s1, 0.0, -d / s1, 0.5 * (W - 1) + mu * p / s2, -p / s2, 0.0),
        270: (0.5 * (H - 1) + mu * p / s1, -p / s1, 0.0, 0.5 * (W - 1) - mj * d / s2, 0.0, d / s2),
    }
    for k, deg in enumerate([0, 90, 180, 270, 0, 270, 90]):
        assert plan.coef[k].tolist() == [float(f(v)) for v in rows[deg]], deg


def test_tables_at_a_general_angle_are_the_fp64_fold_rounded_once():
    H, W, s1, s2 = 9, 6, 2.0, 3.27
    plan = metrics.projection_plan((5, H, W), (3.0, s1, s2), [33.3, 359.0], bins=15, samples=16)
    p = d = 2.0
    for k, deg in enumerate([33.3, 359.0]):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        hu, hj, wu, wj = p * s / s1, d * c / s1, p * c / s2, -d * s / s2
        want = [0.5 * (H - 1) - 7.0 * hu - 7.5 * hj, hu, hj, 0.5 * (W - 1) - 7.0 * wu - 7.5 * wj, wu, wj]
        # the library reduces the angle and evaluates cos and sin itself: a few fp64 ulp, far below fp32's
        assert np.allclose(plan.coef[k].astype(np.float64), want, rtol=2.0 ** -23, atol=2.0 ** -40)


@pytest.mark.parametrize("kwargs, text", [
    (dict(shape=(3, 7), spacing=(1, 1, 1), angles_deg=[0]), "three extents"),
    (dict(shape=(3, 0, 7), spacing=(1, 1, 1), angles_deg=[0]), "three extents"),
    (dict(shape=(3, 7, 13), spacing=(1, 1), angles_deg=[0]), "three positive finite"),
    (dict(shape=(3, 7, 13), spacing=(1, 0, 1), angles_deg=[0]), "three positive finite"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=[]), "1..64 finite angles"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=list(range(65))), "1..64 finite angles"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=[float("nan")]), "1..64 finite angles"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=[0], pitch=0.0), "pitch must be a positive"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=[0], step=float("inf")), "step must be a positive"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=[0], bins=0), "bins must be an integer in 1..4096"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=[0], bins=4097), "bins must be an integer in 1..4096"),
    (dict(shape=(3, 7, 13), spacing=(1, 1, 1), angles_deg=[0], samples=2.5), "samples must be an integer"),
    (dict(shape=(3, 3000, 3000), spacing=(1, 1, 1), angles_deg=[0]), "limited to 4096"),
])
def test_plan_refusals(kwargs, text):
    with pytest.raises(ValueError, match=text):
        metrics.projection_plan(**kwargs)


def test_the_widest_plan_passes():
    plan = metrics.projection_plan((1, 2896, 2896), (1, 1, 1), list(range(64)))
    assert plan.bins == plan.samples == 4096 and plan.coef.shape == (64, 6)
    with pytest.raises(ValueError, match="limited to 4096"):
        metrics.projection_plan((1, 2897, 2896), (1, 1, 1), [0])


# ------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", sorted(PC.EXACT_CASES))
def test_reference_is_amax_and_mirrors_in_the_exact_cases(name):
    case = PC.EXACT_CASES[name]
    vol = PC.volumes(name, 2, case["shape"])
    s = case["spacing"]
    plan = metrics.projection_plan(case["shape"], s, case["angles"], pitch=s[1], step=s[1], bins=case["bins"],
                                   samples=case["samples"])
    out, bound, amb = R.project(vol, plan.coef, plan.bins, plan.samples, plan.table.step, "max")
    assert not amb.any()
    total, total_bound, amb = R.project(vol, plan.coef, plan.bins, plan.samples, plan.table.step, "sum")
    assert not amb.any()
    for k, deg in enumerate(case["angles"]):
        along = 1 if deg in (0.0, 180.0) else 2
        for b in range(2):
            want = PC.amax_image(vol[b], along, plan.bins).astype(np.float64)
            sums = PC.axis_image(vol[b].astype(np.float64).sum(axis=along), plan.bins) * plan.step
            if deg in (180.0, 270.0):
                want, sums = want[:, ::-1], sums[:, ::-1]
            assert np.array_equal(out[b, k], want), (deg, b)
            # every voxel of the column once: step times the column sum, when the ray covers the column
            n = case["shape"][along]
            if plan.samples >= n:
                assert np.allclose(total[b, k], sums, rtol=1e-12, atol=0), (deg, b)
    if 0.0 in case["angles"] and 180.0 in case["angles"]:
        i, j = case["angles"].index(0.0), case["angles"].index(180.0)
        assert np.array_equal(out[:, i], out[:, j, :, ::-1])
    # on a voxel the interpolant is the voxel: the lerp bound alone remains
    assert (bound <= 6.0 * R.U32 * vol.max() * (1 + 2.0 ** -19)).all()


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_reference_max_stays_within_the_volume_and_rows_are_independent(name):
    case = PC.CASES[name]
    vol = PC.volumes(name, max(case["B"], 2), case["shape"])
    plan = _plan(case)
    out, bound, amb = R.project(vol, plan.coef, plan.bins, plan.samples, plan.table.step, "max")
    u, j = np.arange(plan.bins, dtype=np.float64), np.arange(plan.samples, dtype=np.float64)
    for k in range(len(plan.angles_deg)):
        hc = R._coordinate(plan.coef[k, 0:3], u, j)[0]
        wc = R._coordinate(plan.coef[k, 3:6], u, j)[0]
        hit = ((hc >= 0) & (hc <= case["shape"][1] - 1) & (wc >= 0) & (wc <= case["shape"][2] - 1)).any(axis=1)
        for b in range(vol.shape[0]):
            lo = vol[b].min(axis=(1, 2))[:, None]
            hi = vol[b].max(axis=(1, 2))[:, None]
            inside = (out[b, k] >= lo) & (out[b, k] <= hi)
            assert (inside | ~hit[None, :]).all() and (out[b, k][:, ~hit] == 0).all()
    one = R.project(vol[1:2], plan.coef, plan.bins, plan.samples, plan.table.step, "max")
    assert np.array_equal(one[0][0], out[1]) and np.array_equal(one[1][0], bound[1])
    assert (bound >= 0).all() and np.isfinite(bound).all()


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_the_reference_flags_at_most_one_per_cent_of_a_case_ambiguous(name):
    """what lets the GPU tier skip the flagged outputs: they are few, whatever the device does"""
    case = PC.CASES[name]
    vol = PC.volumes(name, case["B"], case["shape"])
    plan = _plan(case)
    for mode in ("max", "sum"):
        amb = R.project(vol, plan.coef, plan.bins, plan.samples, plan.table.step, mode)[2]
        assert amb.mean() <= 0.01, "%s, %s: %d of %d outputs are ambiguous" % (name, mode, amb.sum(), amb.size)


def test_reference_nan_reach():
    plan = metrics.projection_plan((1, 7, 13), (3.0, 2.0, 2.0), [0.0], bins=13, samples=7)
    must, may = R.nan_reach(plan.coef, 13, 7, (7, 13), (3, 5))
    assert must[0].tolist() == [u == 5 for u in range(13)] and may[0].tolist() == [4 <= u <= 6 for u in range(13)]
    vol = np.ones((1, 1, 7, 13))
    vol[0, 0, 3, 5] = np.nan
    for mode in ("max", "sum"):
        out = R.project(vol, plan.coef, 13, 7, plan.table.step, mode)[0]
        # the ray through column 4 has the voxel as its upper corner, with weight 0: NaN all the same; the ray through
        # column 6 does not touch it
        assert np.isnan(out[0, 0, 0]).tolist() == [u in (4, 5) for u in range(13)]


# ------------------------------------------------------------------------------------------ the entries' refusals
def _table(**kw):
    args = dict(H=7, W=13, s1=2.0, s2=2.0, pitch=2.0, bins=13, step=2.0, samples=7, angles=[0.0, 45.0])
    args.update(kw)
    angles = args.pop("angles")
    arr = None if angles is None else (ctypes.c_double * max(len(angles), 1))(*angles)
    table = _hip.ProjectTable()
    n = args.pop("n_angles", 0 if angles is None else len(angles))
    rc = _hip.load().ddpm3d_project_table_fill(args["H"], args["W"], args["s1"], args["s2"], args["pitch"], args["bins"],
                                               args["step"], args["samples"], arr, n, ctypes.byref(table))
    return rc, table


@pytest.mark.parametrize("kw", [
    dict(H=0), dict(W=-1), dict(s1=0.0), dict(s2=float("nan")), dict(pitch=float("inf")), dict(step=-1.0),
    dict(bins=0), dict(bins=4097), dict(samples=0), dict(samples=4097), dict(angles=[]), dict(angles=[0.0] * 65),
    dict(angles=[float("nan")]), dict(angles=[float("inf")]), dict(angles=None, n_angles=1),
    dict(pitch=1e300, s1=1e-300), dict(step=1e39),
], ids=lambda kw: "-".join(sorted(kw)))
def test_table_fill_refusals(kw):
    rc, table = _table(**kw)
    assert rc == _hip.E_INVAL and _hip.load().ddpm3d_last_error().decode().startswith("project_table_fill:")
    assert table.angles == 0 and table.bins == 0                                    # untouched
    lib = _hip.load()
    assert lib.ddpm3d_project_table_fill(7, 13, 2.0, 2.0, 2.0, 13, 2.0, 7, (ctypes.c_double * 1)(0.0), 1, None) \
        == _hip.E_INVAL


def test_project_refusals_return_before_any_launch():
    """no device is present here: a call that got as far as a launch would fail in another way"""
    lib = _hip.load()
    rc, good = _table()
    assert rc == 0
    vol, out = 1 << 20, 1 << 30                             # never dereferenced by a refused call

    def call(vol=vol, B=1, D=3, H=7, W=13, table=good, mode=_hip.PROJECT_MAX, out=out):
        return lib.ddpm3d_project(vol, B, D, H, W, None if table is None else ctypes.byref(table), mode, out, None)

    def edited(**kw):
        t = _hip.ProjectTable()
        ctypes.memmove(ctypes.byref(t), ctypes.byref(good), ctypes.sizeof(t))
        for k, v in kw.items():
            if k == "coef":
                t.coef[v[0]][v[1]] = v[2]
            else:
                setattr(t, k, v)
        return t

    bad = [
        dict(vol=None), dict(out=None), dict(table=None), dict(B=0), dict(B=_hip.MAX_DRAWS + 1), dict(D=0), dict(H=0),
        dict(W=0), dict(mode=2), dict(mode=-1), dict(D=1, H=(1 << 24) + 1, W=1), dict(D=1, H=1, W=(1 << 24) + 1),
        dict(out=vol), dict(out=vol + 4 * 3 * 7 * 13 - 4), dict(out=vol - 4 * 2 * 3 * 13 + 4),
        dict(table=edited(angles=0)), dict(table=edited(angles=65)), dict(table=edited(bins=0)),
        dict(table=edited(bins=4097)), dict(table=edited(samples=0)), dict(table=edited(samples=4097)),
        dict(table=edited(step=float("nan"))), dict(table=edited(coef=(1, 4, float("inf")))),
        dict(table=edited(coef=(0, 0, float("nan")))),
        dict(D=1 << 20, H=1 << 6, W=1 << 5), dict(B=2, D=1 << 15, H=1 << 8, W=1 << 7),    # 2^31 voxels in
        dict(B=64, D=1 << 14, H=1, W=1, table=edited(angles=64, bins=4096)),               # 2^32 out
    ]
    for kw in bad:
        assert call(**kw) == _hip.E_INVAL, kw
        assert lib.ddpm3d_last_error().decode().startswith("project:"), kw


# ------------------------------------------------------------------------------------------ the script's flag
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
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]


MM = ["--voxel_spacing", "3.27", "2", "1.5"]
FINE = ["--voxel_spacing", "3.27", "2", "0.01"]     # a pitch of 0.01 mm: small files reach the bin limit
SCRIPT_CASES = {
    "zero": (["--mip_angles", "0"] + MM, "--mip_angles must be in 1..64", (12, 16, 24)),
    "too_many": (["--mip_angles", "65"] + MM, "--mip_angles must be in 1..64", (12, 16, 24)),
    "no_spacing": (["--mip_angles", "4"], "--mip_angles needs --voxel_spacing", (12, 16, 24)),
    "spacing_two": (["--mip_angles", "4", "--voxel_spacing", "2", "2"], "three numbers", (12, 16, 24)),
    # ceil(hypot(20 * 2, 22 * 0.01) / 0.01) = 4001 bins pass, ceil(hypot(22 * 2, 22 * 0.01) / 0.01) = 4401 do not
    "box_above_4096": (["--mip_angles", "4"] + FINE, "takes 4401 bins; at most 4096", (3, 24, 24)),
    "whole_above_4096": (["--mip_angles", "4", "--joint_patches", "True"] + FINE, "takes 4801 bins; at most 4096",
                         (1, 24, 24)),
    "empty_box": (["--mip_angles", "4"] + MM, "each must be at least 1", (2, 16, 24)),
}


@pytest.mark.parametrize("case", sorted(SCRIPT_CASES))
def test_script_refuses_bad_mip_flags_before_any_device_call(case, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, text, shape = SCRIPT_CASES[case]
    with pytest.raises(SystemExit) as e:
        mod.main(_files(tmp_path, shape) + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err[err.rindex("error:"):]


@pytest.mark.parametrize("flags, shape", [(["--mip_angles", "1"] + MM, (12, 16, 24)),
                                          (["--mip_angles", "64"] + FINE, (3, 22, 24)),
                                          (["--mip_angles", "36", "--joint_patches", "True"] + MM, (1, 16, 24))],
                         ids=["one", "most", "joint"])
def test_script_accepts_good_mip_flags_without_a_target_or_regions(flags, shape, tmp_path, monkeypatch):
    mod = _script()
    _no_device(mod, monkeypatch)
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path, shape) + flags)


def test_script_default_is_no_mip():
    mod = _script()
    args = mod.create_argparser().parse_args([])
    assert args.mip_angles is None and mod._check_mip(None, args) is None and mod._plan_mip(None, args, None) is None
