"""
CPU tier of volume regridding: the fp64 yardstick of tests/regrid_ref.py against torch's trilinear
interpolation and against Pillow's BILINEAR and BICUBIC resize, guided_diffusion/regrid.py's tables against the
yardstick's and their properties, grid_shape, inverse, keep_after's rule against a brute-force set computation, the
two C entries declared, exported and bound within ABI 13, every host refusal of ddpm3d_regrid (no HIP call is made:
the pointers are fake), the Python entries' refusals and the inference script's refusals of bad regrid flags before
any device call.  No GPU is touched here.
"""

import ctypes
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import regrid_ref as R
from conftest import PKG, ROOT
from guided_diffusion import _hip, regrid

FAKE = 1 << 20          # a non-null "device pointer" no call below may ever dereference: each fails validation first


# ------------------------------------------------------------------------------------------ independent references
@pytest.mark.parametrize("shape_out", [(9, 11, 20), (5, 12, 7)], ids=str)
def test_yardstick_equals_torch_trilinear_on_growing_axes(shape_out):
    x = R.data((5, 6, 7), 1).astype(np.float64)
    m, _ = R.apply(x, shape_out, "linear", rounded=False)
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[None, None], size=shape_out, mode="trilinear",
                                           align_corners=False)[0, 0].numpy()
    assert m.shape == shape_out and np.abs(m - want).max() <= 1e-12


@pytest.mark.parametrize("size", [(29, 40), (5, 7), (13, 9), (4, 17)], ids=str)
@pytest.mark.parametrize("mode", ["linear", "cubic"])
def test_yardstick_equals_pillow(mode, size):
    x = R.data((13, 17), 2)
    m, _ = R.apply(x[None], (1,) + size, mode, rounded=False)
    resample = Image.BILINEAR if mode == "linear" else Image.BICUBIC
    want = np.asarray(Image.fromarray(x).resize(size[::-1], resample), dtype=np.float64)
    assert want.shape == size and np.abs(m[0] - want).max() <= 1e-6


# ------------------------------------------------------------------------------------------ the tables
PAIRS = [(7, 20), (20, 7), (19, 6), (6, 19), (5, 20), (20, 5), (68, 17), (17, 68), (1, 3), (3, 1), (1, 4), (33, 11),
         (64, 257), (257, 64), (2, 3)]


@pytest.mark.parametrize("mode", ["linear", "cubic"])
@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_tables_equal_the_yardsticks_and_rows_sum_to_one(pair, mode):
    Li, Lo = pair
    t = regrid.axis_table(Li, Lo, mode)
    first, count, rows = R.table(Li, Lo, mode)
    assert t.first.tolist() == first and t.count.tolist() == count and t.taps == max(count)
    assert (t.in_len, t.out_len, t.scale) == (Li, Lo, Li / Lo)
    assert t.weights64.shape == t.weights.shape == (Lo, t.taps) and t.weights.dtype == np.float32
    for o in range(Lo):
        assert np.abs(t.weights64[o, :count[o]] - np.asarray(rows[o])).max() <= 1e-15
        assert (t.weights64[o, count[o]:] == 0).all() and count[o] >= 1
        assert abs(t.weights64[o].sum() - 1.0) <= 4e-16 * count[o]
        assert first[o] >= 0 and first[o] + count[o] <= Li
    assert np.array_equal(t.weights, t.weights64.astype(np.float32))
    M, n = R.matrix(Li, Lo, mode)
    dense = np.zeros((Lo, Li))
    for o in range(Lo):
        dense[o, first[o]:first[o] + count[o]] = t.weights[o, :count[o]]
    assert np.array_equal(M, dense) and n.tolist() == count
    if mode == "linear":
        assert (t.weights64 >= 0).all()


def test_tap_counts_stay_within_the_limit_at_both_ends_of_the_ratio():
    assert _hip.REGRID_MAX_TAPS == R.MAX_TAPS == 18
    # int(c + S fs + 0.5) - int(c - S fs + 0.5) is 2 S fs when that is whole: 16 for cubic at ratio 4, one below the
    # 2 S fs + 1 = 17 a window of that width could hold, and within the 18 the entry allows
    for Lo in (1, 2, 3, 17, 50):
        assert regrid.axis_table(4 * Lo, Lo, "cubic").taps <= 17 <= _hip.REGRID_MAX_TAPS
        assert regrid.axis_table(4 * Lo, Lo, "linear").taps <= 9
        assert regrid.axis_table(Lo, 4 * Lo, "cubic").taps <= 4            # ratio 1/4: the kernel is not widened
        assert regrid.axis_table(Lo, 4 * Lo, "linear").taps <= 2
    assert regrid.axis_table(68, 17, "cubic").taps == 16 and regrid.axis_table(68, 17, "linear").taps == 8
    assert max(regrid.axis_table(Li, Lo, "cubic").taps for Li in range(1, 70) for Lo in range(1, 70)
               if 0.25 <= Li / Lo <= 4 and Li != Lo) <= 17


@pytest.mark.parametrize("mode", ["linear", "cubic"])
def test_unit_extent_gives_one_tap_of_weight_one(mode):
    for Lo in (2, 3, 4):
        t = regrid.axis_table(1, Lo, mode)
        assert t.taps == 1 and t.first.tolist() == [0] * Lo and t.count.tolist() == [1] * Lo
        assert t.weights.tolist() == [[1.0]] * Lo
    t = regrid.axis_table(4, 1, mode)
    assert t.count.tolist() == [4] and t.first.tolist() == [0] and abs(t.weights64.sum() - 1.0) < 1e-15
    t = regrid.axis_table(6, 6, mode)
    assert t.identity and t.taps == 0 and t.weights.shape == (6, 0)


def test_grid_shape_rounds_to_the_nearest_voxel_count():
    assert regrid.grid_shape((12, 20, 20), (4.0, 4.0, 4.0), (2.0, 2.0, 2.0)) == (24, 40, 40)
    assert regrid.grid_shape((130, 200, 200), (3.27, 2.0, 2.0), (2.0, 2.0, 2.0)) == (213, 200, 200)   # 212.55
    assert regrid.grid_shape((10, 10, 10), (2.0, 2.0, 2.0), (3.0, 8.0, 40.0)) == (7, 3, 1)            # 6.67, 2.5, 0.5
    assert regrid.grid_shape((10, 10, 1), (2.0, 2.0, 2.0), (2.1, 1.9, 100.0)) == (10, 11, 1)          # at least 1
    assert regrid.grid_shape((5, 6, 7), (2.0, 3.0, 4.0), (2.0, 3.0, 4.0)) == (5, 6, 7)
    for bad in ((0.0, 2, 2), (2, 2), (2, -1, 2), (2, float("nan"), 2), (2, 2, float("inf")), "222", None):
        with pytest.raises(ValueError, match="regrid:"):
            regrid.grid_shape((5, 6, 7), bad, (2, 2, 2))
        with pytest.raises(ValueError, match="regrid:"):
            regrid.grid_shape((5, 6, 7), (2, 2, 2), bad)
    for bad in ((5, 6), (5, 0, 7), (5, 6, 7, 8), None, (2048, 1024, 1024)):
        with pytest.raises(ValueError, match="regrid:"):
            regrid.grid_shape(bad, (2, 2, 2), (2, 2, 2))


def test_plan_inverse_absolute_and_refusals():
    p = regrid.plan((12, 9, 33), (12, 20, 11), "cubic")
    assert (p.shape_in, p.shape_out, p.mode) == ((12, 9, 33), (12, 20, 11), "cubic")
    assert p.scale == (1.0, 9 / 20, 3.0) and [a.identity for a in p.axes] == [True, False, False] and not p.identity
    q = p.inverse()
    assert (q.shape_in, q.shape_out, q.mode) == ((12, 20, 11), (12, 9, 33), "cubic") and q.inverse() is p
    assert q.scale == (1.0, 20 / 9, 1 / 3)
    a = p.absolute()
    assert (a.shape_in, a.shape_out) == (p.shape_in, p.shape_out) and p.absolute() is a
    assert (p.axes[2].weights < 0).any()
    for x, y in zip(p.axes, a.axes):
        assert np.array_equal(y.weights, np.abs(x.weights)) and np.array_equal(y.weights64, np.abs(x.weights64))
        assert np.array_equal(y.first, x.first) and np.array_equal(y.count, x.count) and y.taps == x.taps
    assert regrid.plan((5, 6, 7), (5, 6, 7)).identity and regrid.plan((5, 6, 7), (5, 6, 7)).mode == "linear"
    with pytest.raises(ValueError, match="unknown mode 'nearest'"):
        regrid.plan((5, 6, 7), (5, 6, 7), "nearest")
    with pytest.raises(ValueError, match=r"axis H: 6 -> 25 voxels.*outside \[1/4, 4\]"):
        regrid.plan((5, 6, 7), (5, 25, 7))
    with pytest.raises(ValueError, match=r"axis W: 29 -> 7"):
        regrid.plan((5, 6, 29), (5, 6, 7))
    with pytest.raises(ValueError, match="axis D"):
        regrid.plan((1, 6, 7), (5, 6, 7))
    assert regrid.plan((1, 6, 28), (4, 6, 7)).scale == (0.25, 1.0, 4.0)
    for bad in ((5, 6), (5, 0, 7), None, (2048, 1024, 1024)):
        with pytest.raises(ValueError, match="regrid:"):
            regrid.plan(bad, (5, 6, 7))
        with pytest.raises(ValueError, match="regrid:"):
            regrid.plan((5, 6, 7), bad)


@pytest.mark.parametrize("mode", ["linear", "cubic"])
def test_keep_after_rule_against_a_brute_force_set_computation(mode):
    shape_in, shape_out = (6, 5, 9), (4, 5, 13)
    keep = np.ones(shape_in, dtype=np.uint8)
    keep[0], keep[:, :, -1], keep[3, 2, 4] = 0, 0, 0
    got = R.keep_after(keep, shape_out, mode)
    p = regrid.plan(shape_in, shape_out, mode)
    enters = []                                    # per axis and output index: the inputs with a non-zero fp32 tap
    for a in p.axes:
        if a.identity:
            enters.append([{o} for o in range(a.out_len)])
        else:
            enters.append([{int(a.first[o]) + t for t in range(int(a.count[o])) if a.weights[o, t] != 0}
                           for o in range(a.out_len)])
    want = np.zeros(shape_out, dtype=np.uint8)
    for z, y, x in itertools.product(*(range(n) for n in shape_out)):
        want[z, y, x] = all(keep[k] for k in itertools.product(enters[0][z], enters[1][y], enters[2][x]))
    assert np.array_equal(got, want) and 0 < want.sum() < want.size
    assert not want[0].any() and not want[:, :, -1].any() and want[2, 2, 2] == 1
    # and a NaN reaches the outputs that count it as a tap, whatever its weight: a superset of the above
    bad = np.zeros(shape_in, dtype=bool)
    bad[3, 2, 4] = True
    reach = R.nonfinite_after(bad, shape_out, mode)
    hole = R.keep_after((~bad).astype(np.uint8), shape_out, mode) == 0
    assert reach.any() and (reach | ~hole).all()


def test_yardstick_bound_on_a_case_worked_by_hand():
    x = np.array([1.0, 3.0], dtype=np.float32).reshape(1, 1, 2)
    m, e = R.apply(x, (1, 1, 4), "linear")
    assert m[0, 0].tolist() == pytest.approx([1.0, 1.5, 2.5, 3.0], rel=1e-7)     # 0.75 / 0.25 weights, fp32-rounded
    g1, g2 = R.U / (1 - R.U), 2 * R.U / (1 - 2 * R.U)
    assert e[0, 0].tolist() == pytest.approx([g1 * 1.0, g2 * 1.5, g2 * 2.5, g1 * 3.0], rel=1e-7)
    # two passes compose: e_2 = |W| e_1 + gamma |W| (|m_1| + e_1)
    y = np.array([[1.0, 3.0], [5.0, 7.0]], dtype=np.float32).reshape(1, 2, 2)
    m2, e2 = R.apply(y, (1, 4, 4), "linear")
    m1, e1 = R.apply(y, (1, 2, 4), "linear")
    A = np.abs(R.matrix(2, 4, "linear")[0])
    want = A @ e1[0] + R.gamma([1, 2, 2, 1])[:, None] * (A @ (np.abs(m1[0]) + e1[0]))
    assert np.allclose(e2[0], want, rtol=1e-12, atol=0) and (e2 > 0).all()


# ------------------------------------------------------------------------------------------ the C entries
NAMES = ("ddpm3d_regrid_workspace_bytes", "ddpm3d_regrid")


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ddpm3d.h")).read()
    declared = set(re.findall(r"\b(ddpm3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define DDPM3D_ABI_VERSION 13\b", hdr) and _hip.load().ddpm3d_abi_version() == 13
    assert int(re.search(r"#define DDPM3D_REGRID_MAX_TAPS (\S+)", hdr).group(1)) == _hip.REGRID_MAX_TAPS == 18
    assert re.search(r"typedef struct ddpm3d_regrid_axis \{", hdr)
    assert [f[0] for f in _hip.RegridAxis._fields_] == ["in_len", "out_len", "taps", "first", "count", "weights"]
    assert ctypes.sizeof(_hip.RegridAxis) == 40
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*:=.*\bregrid\.o\b", make, re.M)
    assert os.path.isfile(os.path.join(PKG, "csrc", "regrid.hip"))
    lib = _hip.load()
    # the W pass's and the H pass's outputs, each rounded up to 16 bytes
    a16 = lambda n: (n + 15) // 16 * 16
    assert lib.ddpm3d_regrid_workspace_bytes(1, 5, 6, 7, 9, 11, 20) == a16(5 * 6 * 20 * 4) + a16(5 * 11 * 20 * 4)
    assert lib.ddpm3d_regrid_workspace_bytes(3, 5, 6, 7, 9, 11, 20) == a16(3 * 5 * 6 * 20 * 4) + a16(3 * 5 * 11 * 20 * 4)
    assert lib.ddpm3d_regrid_workspace_bytes(1, 1, 1, 1, 1, 1, 1) == 32
    for bad in ((0, 5, 6, 7, 9, 11, 20), (65, 5, 6, 7, 9, 11, 20), (1, 0, 6, 7, 9, 11, 20), (1, 5, 6, 7, 9, 11, 0),
                (1, 5, 6, 7, 9, 11, 29), (1, 5, 6, 7, 21, 11, 20), (1, 5, 25, 7, 5, 6, 7),
                (1, 2048, 1024, 1024, 2048, 1024, 1024), (1, 1024, 1024, 1024, 1024, 1024, 4096)):
        assert lib.ddpm3d_regrid_workspace_bytes(*bad) == 0, bad


def _axes(shape_in, shape_out, taps=(2, 2, 2), **over):
    arr = (_hip.RegridAxis * 3)()
    for i in range(3):
        same = shape_in[i] == shape_out[i]
        arr[i].in_len, arr[i].out_len, arr[i].taps = shape_in[i], shape_out[i], 0 if same else taps[i]
        arr[i].first, arr[i].count, arr[i].weights = 4 * FAKE, 5 * FAKE, 6 * FAKE
    for key, value in over.items():
        i, field = int(key[1]), key[3:]
        setattr(arr[i], field, value)
    return arr


def _regrid(shape_in=(5, 6, 7), shape_out=(9, 6, 20), **over):
    lib = _hip.load()
    need = 1 << 16
    a = dict(vol=FAKE, B=2, D=shape_in[0], H=shape_in[1], W=shape_in[2], axes=None, out=2 * FAKE, ws=3 * FAKE,
             ws_bytes=need, stream=None)
    axis_over = {k: over.pop(k) for k in list(over) if re.match(r"a\d_", k)}
    a.update(over)
    if a["axes"] is None and "no_axes" not in over:
        a["axes"] = _axes(shape_in, shape_out, **axis_over)
    a.pop("no_axes", None)
    rc = lib.ddpm3d_regrid(*a.values())
    return rc, lib.ddpm3d_last_error().decode()


WS_NEED = ((2 * 5 * 6 * 20 * 4 + 15) // 16 * 16) * 2          # B = 2, (5, 6, 7) -> (9, 6, 20): H is the identity
BAD_REGRID = {
    "vol_null": (dict(vol=None), "null"), "out_null": (dict(out=None), "null"),
    "axes_null": (dict(no_axes=True), "null"),
    "first_null": (dict(a0_first=None), "axes[0] (D): null"), "count_null": (dict(a2_count=None), "axes[2] (W): null"),
    "weights_null": (dict(a2_weights=None), "axes[2] (W): null"),
    "B_0": (dict(B=0), "B=0"), "B_65": (dict(B=65), "B=65"),
    "D_0": (dict(D=0, a0_in_len=0), "in_len=0"), "W_negative": (dict(W=-7, a2_in_len=-7), "in_len=-7"),
    "out_len_0": (dict(a1_out_len=0), "out_len=0"),
    "taps_negative": (dict(a0_taps=-1), "taps=-1"), "taps_19": (dict(a2_taps=19), "taps=19"),
    "identity_lengths_differ": (dict(a0_taps=0), "identity"),
    "in_len_not_the_shape": (dict(a2_in_len=8), "the volume has W=7"),
    "in_len_not_the_shape_D": (dict(a0_in_len=4), "the volume has D=5"),
    "ratio_above_4": (dict(a2_out_len=1), "ratio in_len / out_len = 7 / 1"),
    "ratio_below_quarter": (dict(a0_out_len=21), "ratio in_len / out_len = 5 / 21"),
    "voxels_2_31": (dict(shape_in=(2048, 1024, 1024), shape_out=(2048, 1024, 1025)), "2^31 - 1"),
    "voxels_after_a_pass": (dict(shape_in=(1024, 1024, 1024), shape_out=(1024, 1024, 4096)), "2^31 - 1"),
    "ws_null": (dict(ws=None), "workspace"), "ws_small": (dict(ws_bytes=WS_NEED - 1), "workspace"),
    "ws_misaligned": (dict(ws=3 * FAKE + 4), "workspace"),
    "ws_overlaps_vol": (dict(ws=FAKE + 16), "workspace overlaps"),
    "ws_overlaps_out": (dict(ws=2 * FAKE - 16), "workspace overlaps"),
    "in_place": (dict(out=FAKE), "out overlaps vol"),
    "out_inside_vol": (dict(out=FAKE + 2 * 5 * 6 * 7 * 4 - 4), "out overlaps vol"),
    "vol_inside_out": (dict(out=FAKE - 2 * 9 * 6 * 20 * 4 + 4), "out overlaps vol"),
}


@pytest.mark.parametrize("case", sorted(BAD_REGRID))
def test_regrid_refuses_bad_arguments_and_names_them(case):
    over, names = BAD_REGRID[case]
    rc, msg = _regrid(**dict(over))
    assert rc == _hip.E_INVAL and msg.startswith("regrid:") and names in msg, (rc, msg)


def test_the_last_refusal_is_the_workspace_size():
    """with everything else in order the entry gets as far as the workspace check: the refusals above are each
    argument's own"""
    rc, msg = _regrid(ws_bytes=WS_NEED - 1)
    assert rc == _hip.E_INVAL and "needs %d bytes" % WS_NEED in msg
    assert _hip.load().ddpm3d_regrid_workspace_bytes(2, 5, 6, 7, 9, 6, 20) == WS_NEED


# ------------------------------------------------------------------------------------------ the Python entries
def test_python_refusals_come_before_the_library(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a refusal reached the library")

    monkeypatch.setattr(regrid.H, "load", no_device)
    p = regrid.plan((4, 5, 6), (8, 5, 3))
    vol = torch.zeros((4, 5, 6))
    for bad in (vol, vol.numpy(), None):
        with pytest.raises(ValueError, match="regrid.apply: volume must live on the GPU"):
            regrid.apply(bad, p)
    with pytest.raises(ValueError, match="plan must be regrid.plan's return"):
        regrid.apply(vol, ((4, 5, 6), (8, 5, 3)))
    keep = torch.ones((4, 5, 6), dtype=torch.uint8)
    with pytest.raises(ValueError, match="regrid.keep_after: keep must live on the GPU"):
        regrid.keep_after(keep, p)


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
    return ["--base_samples", str(tmp_path / "low.npz"), "--save_dir", str(tmp_path)]


def test_script_default_is_no_regridding():
    mod = _script()
    parser = mod.create_argparser()
    args = parser.parse_args([])
    assert args.model_spacing is None and args.regrid_mode == "linear"
    mod._check_regrid(parser, args)
    assert args.regrid is None and mod._plan_regrid(parser, args, None) is None and not mod._regridding(args)


SPACING = ["--voxel_spacing", "4", "4", "4"]
MODEL = ["--model_spacing", "2", "2", "2"]
CASES = {
    "no_voxel_spacing": (MODEL, "--model_spacing needs --voxel_spacing"),
    "two_numbers": (SPACING + ["--model_spacing", "2", "2"], "--model_spacing takes three numbers"),
    "four_numbers": (SPACING + ["--model_spacing", "2", "2", "2", "2"], "--model_spacing takes three numbers"),
    "zero": (SPACING + ["--model_spacing", "2", "0", "2"], "positive finite"),
    "negative": (SPACING + ["--model_spacing", "-2", "2", "2"], "positive finite"),
    "nan": (SPACING + ["--model_spacing", "2", "2", "nan"], "positive finite"),
    "inf": (SPACING + ["--model_spacing", "inf", "2", "2"], "positive finite"),
    "not_a_number": (SPACING + ["--model_spacing", "two", "2", "2"], "--model_spacing"),
    "voxel_spacing_two_numbers": (["--voxel_spacing", "4", "4"] + MODEL, "--voxel_spacing takes three numbers"),
    "ratio_above_4_along_H": (SPACING + ["--model_spacing", "4", "20", "4"], "axis H"),
    "ratio_below_quarter_along_D": (SPACING + ["--model_spacing", "0.9", "4", "4"], "axis D"),
    "ratio_above_4_along_W": (SPACING + ["--model_spacing", "4", "4", "20"], "axis W"),
    "unknown_mode": (SPACING + MODEL + ["--regrid_mode", "nearest"], "--regrid_mode must be linear or cubic"),
    "unknown_mode_alone": (["--regrid_mode", "lanczos"], "--regrid_mode must be linear or cubic"),
    "trace": (SPACING + MODEL + ["--trace", "True"], "--trace True cannot be combined with --model_spacing"),
    "no_such_file": (SPACING + MODEL + ["--base_samples", "/nonexistent/pet.npz"], "no such file"),
    # without --model_spacing the spacing's own refusals stand
    "voxel_spacing_alone_no_target": (SPACING, "--voxel_spacing needs --target_samples"),
}


NO_TARGET_ONLY = ("voxel_spacing_alone_no_target", "no_such_file")     # with a target these are other refusals


@pytest.mark.parametrize("case,with_target", [(c, t) for c in sorted(CASES) for t in (False, True)
                                              if not (t and c in NO_TARGET_ONLY)])
def test_script_refuses_bad_regrid_flags_before_any_device_call(case, with_target, tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    extra, names = CASES[case]
    argv = _files(tmp_path) + extra + (["--target_samples", str(tmp_path / "full.npz")] if with_target else [])
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert names in err[err.rindex("error:"):]                # the message itself, not the usage lines above it


def test_voxel_spacing_with_a_target_but_no_regions_is_still_refused(tmp_path, monkeypatch, capsys):
    mod = _script()
    _no_device(mod, monkeypatch)
    with pytest.raises(SystemExit):
        mod.main(_files(tmp_path) + SPACING + ["--target_samples", str(tmp_path / "full.npz")])
    err = capsys.readouterr().err
    assert "--voxel_spacing needs regions" in err[err.rindex("error:"):]


@pytest.mark.parametrize("flags", [SPACING + MODEL, SPACING + MODEL + ["--regrid_mode", "cubic"],
                                   SPACING + ["--model_spacing", "4", "4", "4"],
                                   SPACING + ["--model_spacing", "1", "16", "3.3", "--num_draws", "2"],
                                   SPACING + MODEL + ["--patch_overlap", "6", "--device_noise", "True"],
                                   SPACING + MODEL + ["--joint_patches", "True", "--use_ddim", "True"]],
                         ids=["linear", "cubic", "identity", "limits-draws", "sliding-keyed", "joint-ddim"])
@pytest.mark.parametrize("with_target", [False, True], ids=["no-target", "target"])
def test_script_accepts_good_regrid_flags_before_it_builds_the_model(flags, with_target, tmp_path, monkeypatch):
    """the same set-up with nothing wrong reaches the first device call, with or without a target and with no
    regions: the refusals above are the checks' own"""
    mod = _script()
    _no_device(mod, monkeypatch)
    target = ["--target_samples", str(tmp_path / "full.npz")] if with_target else []
    with pytest.raises(AssertionError, match="went past its argument checks"):
        mod.main(_files(tmp_path) + flags + target + ["--large_size", "16"])


def test_script_plans_on_the_files_axes(tmp_path):
    mod = _script()
    parser = mod.create_argparser()
    args = parser.parse_args(_files(tmp_path) + ["--voxel_spacing", "3.27", "4", "2", "--model_spacing", "2", "2", "2",
                                                 "--regrid_mode", "cubic"])
    mod._check_regrid(parser, args)
    assert mod._check_spacing(parser, args) is None           # no target, no regions: the spacing serves the regridding
    vol = mod._plan_regrid(parser, args, None)
    plan = args.regrid["plan"]
    assert vol.shape == (12, 16, 24) and args.regrid["native"] is vol
    assert plan.shape_in == (12, 16, 24) and plan.shape_out == (20, 32, 24) and plan.mode == "cubic"   # 19.62 -> 20
    assert [a.identity for a in plan.axes] == [False, False, True] and mod._regridding(args)
