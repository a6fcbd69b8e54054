"""
GPU tier of the rotating maximum-intensity and ray-sum projections: ddpm3d_project on every case
of tests/projection_cases.py, both modes, output by output within the header's bound of the fp64 yardstick
(tests/projection_ref.py; the outputs it flags ambiguous, at most 1 % by the CPU tier, are skipped and counted), the
exact cases bit for bit against torch.amax and 0 against 180 degrees, batch independence and repeatability, one NaN
voxel, metrics.project's two input ranks, and the inference script's --mip_angles.

Fraction of the bound used, one run on one board (largest error / bound over the unflagged outputs): 0.645 in max
and 0.368 in sum mode (1 x 4 x 5, 64 angles), at most 0.39 / 0.30 in every other case; 4 of 8448 outputs flagged in
that case, none elsewhere.
"""

import numpy as np
import pytest
import torch

import projection_cases as PC
import projection_ref as R
from guided_diffusion import _hip, metrics, tiff_io

pytestmark = pytest.mark.gpu

MODES = ("max", "sum")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _plan(case):
    return metrics.projection_plan(case["shape"], case["spacing"], PC.angles_of(case), **case["plan"])


_REF = {}


def _reference(name, mode):
    """computed once per (case, mode) and shared; never written to"""
    if (name, mode) not in _REF:
        case = PC.CASES[name]
        plan = _plan(case)
        vol = PC.volumes(name, case["B"], case["shape"])
        ref = R.project(vol, plan.coef, plan.bins, plan.samples, plan.table.step, mode)
        for a in ref:
            a.setflags(write=False)
        _REF[name, mode] = (plan, vol) + ref
    return _REF[name, mode]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_every_unflagged_output_is_within_the_bound(name, mode):
    plan, vol, want, bound, ambiguous = _reference(name, mode)
    got = metrics.project(dev(vol), plan, mode=mode).cpu().numpy().astype(np.float64)
    assert got.shape == want.shape == (vol.shape[0], len(plan.angles_deg), vol.shape[1], plan.bins)
    err = np.abs(got - want)
    keep = ~ambiguous
    used = float(np.max(np.where(keep & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
    print("%s, %s: %d of %d outputs skipped as ambiguous, largest error / bound %.4f, largest bound %.3e"
          % (name, mode, ambiguous.sum(), ambiguous.size, used, bound.max()))
    assert np.isfinite(got).all()
    worst = np.unravel_index(np.argmax(np.where(keep, err - bound, -np.inf)), err.shape)
    assert (err[keep] <= bound[keep]).all(), (
        "%s, %s: output %s is off by %.3e, the bound is %.3e (%d of %d outputs skipped as ambiguous)"
        % (name, mode, worst, err[worst], bound[worst], ambiguous.sum(), ambiguous.size))
    # a ray that misses the slice gives exactly 0 in both modes
    missed = keep & (want == 0) & (bound == 0)
    assert (got[missed] == 0).all()


@pytest.mark.parametrize("name", sorted(PC.EXACT_CASES))
def test_exact_cases_are_torch_amax_bit_for_bit(name):
    case = PC.EXACT_CASES[name]
    s = case["spacing"]
    vol = dev(PC.volumes(name, 2, case["shape"]))
    plan = metrics.projection_plan(case["shape"], s, case["angles"], pitch=s[1], step=s[1], bins=case["bins"],
                                   samples=case["samples"])
    got = metrics.project(vol, plan, mode="max")
    for k, deg in enumerate(case["angles"]):
        along = 1 if deg in (0.0, 180.0) else 2
        best = torch.amax(vol, dim=along + 1)                                   # (B, D, n)
        n = best.shape[-1]
        want = torch.zeros((2, case["shape"][0], plan.bins), dtype=torch.float32, device=vol.device)
        first = (plan.bins - n) // 2
        lo, hi = max(first, 0), min(first + n, plan.bins)
        want[..., lo:hi] = best[..., lo - first:hi - first]
        if deg in (180.0, 270.0):
            want = want.flip(-1)
        assert torch.equal(got[:, k], want), deg
    if 0.0 in case["angles"] and 180.0 in case["angles"]:
        i, j = case["angles"].index(0.0), case["angles"].index(180.0)
        assert torch.equal(got[:, i], got[:, j].flip(-1))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["3x7x13_25_even_odd", "5x9x6_iso_default", "1x4x5_64_angles"])
def test_rows_do_not_depend_on_the_batch_and_two_runs_give_the_same_bits(name, mode):
    plan, vol, _, _, _ = _reference(name, mode)
    x = dev(vol)
    first = metrics.project(x, plan, mode=mode)
    assert torch.equal(metrics.project(x, plan, mode=mode), first)
    for b in range(vol.shape[0]):
        assert torch.equal(metrics.project(x[b].contiguous(), plan, mode=mode), first[b]), b
        assert torch.equal(metrics.project(x[b:b + 1].contiguous(), plan, mode=mode)[0], first[b]), b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name, voxel", [("3x7x13_iso_default", (1, 3, 5)), ("5x9x6_327_odd_even", (4, 8, 0)),
                                         ("3x7x13_327_fine", (0, 0, 12))])
def test_one_nan_voxel(name, voxel, mode):
    plan, vol, _, _, _ = _reference(name, mode)
    vol = vol[:1].copy()
    clean = metrics.project(dev(vol), plan, mode=mode).cpu().numpy()
    vol[0][voxel] = np.nan
    got = metrics.project(dev(vol), plan, mode=mode).cpu().numpy()
    must, may = R.nan_reach(plan.coef, plan.bins, plan.samples, vol.shape[2:], voxel[1:])
    d = voxel[0]
    assert must.any() and not may.all()
    assert np.isnan(got[0, :, d, :][must]).all()
    assert np.array_equal(got[0, :, d, :][~may], clean[0, :, d, :][~may])
    others = [z for z in range(vol.shape[1]) if z != d]
    assert np.array_equal(got[0][:, others], clean[0][:, others])              # the other slices never see it


def test_project_takes_one_volume_or_a_stack_and_refuses_the_rest():
    plan = metrics.projection_plan((3, 7, 13), (3.0, 2.0, 2.0), [0.0, 30.0])
    vol = dev(PC.volumes("ranks", 2, (3, 7, 13)))
    one, stack = metrics.project(vol[0], plan), metrics.project(vol, plan, mode="sum")
    assert one.shape == (2, 3, plan.bins) and stack.shape == (2, 2, 3, plan.bins)
    assert one.is_cuda and one.dtype == torch.float32 and stack.is_contiguous()
    for bad, text in ((vol[:, :2], "against a plan"), (vol[0, 0], "against a plan")):
        with pytest.raises(ValueError, match=text):
            metrics.project(bad.contiguous(), plan)
    with pytest.raises(ValueError, match="mode"):
        metrics.project(vol, plan, mode="mean")
    with pytest.raises(ValueError, match="projection_plan's return"):
        metrics.project(vol, None)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.project(vol.cpu(), plan)
    # the entry's own refusal of overlapping buffers, on real device memory
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    rc = _hip.load().ddpm3d_project(buf.data_ptr(), 1, 3, 7, 13, plan.table, _hip.PROJECT_MAX, buf.data_ptr() + 64,
                                    _hip.stream())
    assert rc == _hip.E_INVAL and "overlaps" in _hip.load().ddpm3d_last_error().decode()


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
MM = (3.27, 2.0, 1.5)                                                      # along the file's (D, H, W)


def _script():
    import importlib.util
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import metrics_ref
    d = tmp_path_factory.mktemp("mip")
    target = metrics_ref.phantom((24, 40, 40), seed=4)
    low = metrics_ref.noisy(target, 0.1, seed=4)
    np.savez(d / "pet.npz", low)
    np.savez(d / "full.npz", target)
    tiff_io.imwrite(str(d / "pet.tif"), low.astype(np.float32))
    return d, target, low


def _mip(volume_dhw, box, angles):
    lo, hi = box
    cut = np.ascontiguousarray(volume_dhw[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], dtype=np.float32)
    plan = metrics.projection_plan(cut.shape, MM, angles)
    return metrics.project(dev(cut), plan).cpu().numpy(), plan


def test_script_writes_the_mip_of_every_row_and_nothing_else_changes(files):
    d, target, low = files
    mod = _script()
    common = FLAGS + ["--base_samples", str(d / "pet.npz"), "--target_samples", str(d / "full.npz"),
                      "--voxel_spacing"] + [repr(s) for s in MM] + ["--baseline_gaussian_fwhm", "5", "--num_draws", "2"]
    mod.main(common + ["--save_dir", str(d / "with"), "--mip_angles", "4"])
    mod.main(common + ["--save_dir", str(d / "plain")])
    z = np.load(d / "with" / "mip_pet.npz")
    assert z.files == ["denoised", "input", "target", "error", "std", "gaussian", "angles_deg", "pitch_mm"]
    assert z["angles_deg"].tolist() == [0.0, 90.0, 180.0, 270.0] and float(z["pitch_mm"]) == 1.5
    written = np.load(d / "with" / "denoised_pet.npz")
    den, std = written["arr_0"].transpose(2, 0, 1), written["std"].transpose(2, 0, 1)   # (H, W, Z) -> (D, H, W)
    box = ([1, 1, 1], [23, 39, 39])
    want, plan = _mip(den, box, z["angles_deg"].tolist())
    assert z["denoised"].dtype == np.float32 and z["denoised"].shape == (4, 22, plan.bins) == want.shape
    assert np.array_equal(z["denoised"], want)
    assert np.array_equal(z["input"], _mip(low, box, z["angles_deg"].tolist())[0])
    assert np.array_equal(z["target"], _mip(target, box, z["angles_deg"].tolist())[0])
    assert np.array_equal(z["std"], _mip(std, box, z["angles_deg"].tolist())[0])
    error = (dev(den.astype(np.float32)) - dev(target.astype(np.float32))).abs().cpu().numpy()
    assert np.array_equal(z["error"], _mip(error, box, z["angles_deg"].tolist())[0])
    smooth = metrics.gaussian_smooth(dev(low.astype(np.float32).transpose(1, 2, 0)),
                                     metrics.gaussian_taps(5.0, (MM[1], MM[2], MM[0]))).permute(2, 0, 1).cpu().numpy()
    assert np.array_equal(z["gaussian"], _mip(smooth, box, z["angles_deg"].tolist())[0])
    assert z["denoised"].max() > 0 and not np.array_equal(z["denoised"], z["input"])
    # the same run without the flag: the .npz and the metrics file byte for byte, the log but for the MIP's line
    for name in ("denoised_pet.npz", "metrics_pet.json"):
        assert open(d / "plain" / name, "rb").read() == open(d / "with" / name, "rb").read(), name
    assert not (d / "plain" / "mip_pet.npz").exists() and not (d / "with" / "mip_pet.tif").exists()
    log = open(d / "with" / "log.txt").read().replace(str(d / "with"), str(d / "plain")).splitlines()
    mine = [line for line in log if "maximum-intensity" in line]
    assert len(mine) == 1 and "denoised, input, target, error, std, gaussian" in mine[0]
    assert [line for line in log if line not in mine] == open(d / "plain" / "log.txt").read().splitlines()


def test_script_mip_of_a_tif_on_the_joint_path_needs_no_target(files):
    d, target, low = files
    mod = _script()
    mod.main(FLAGS + ["--base_samples", str(d / "pet.tif"), "--save_dir", str(d / "tif"), "--joint_patches", "True",
                      "--voxel_spacing"] + [repr(s) for s in MM] + ["--mip_angles", "3"])
    z = np.load(d / "tif" / "mip_pet.npz")
    assert z.files == ["denoised", "input", "angles_deg", "pitch_mm"]
    assert z["angles_deg"].tolist() == [0.0, 120.0, 240.0]
    den = np.load(d / "tif" / "denoised_pet.npz")["arr_0"].transpose(2, 0, 1)
    box = ([0, 0, 0], [24, 40, 40])                                         # the joint path: the whole volume
    want, plan = _mip(den, box, z["angles_deg"].tolist())
    assert z["denoised"].shape == (3, 24, plan.bins) and np.array_equal(z["denoised"], want)
    assert np.array_equal(z["input"], _mip(low, box, z["angles_deg"].tolist())[0])
    back = tiff_io.imread(str(d / "tif" / "mip_pet.tif"))
    assert back.dtype == np.float32 and np.array_equal(back, z["denoised"])
    assert not (d / "tif" / "metrics_pet.json").exists()
