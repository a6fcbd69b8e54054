"""
The bits of every entry that reduces a volume to fp64 records (csrc/record_reduce.h): error moments,
trace moments, the variational bound's terms and prior, per-region moments, SSIM and multi-scale SSIM.  The other tests
hold these entries to fp64 restatements within a tolerance; this one pins the ORDER of the reduction: every output is
compared, as integer bit patterns (so NaN counts too), to tests/golden/moment_records.npz, which was recorded once
from the library as it stood before the shared reduction replaced the per-entry copies (commit 63e213e) and is never
regenerated from newer code.  The shapes are the smallest at which each path can go wrong (1024 values per pass, folds of 256 threads,
part caps of 2048 and 1024): more than 256 records per fold, both load paths, a capped plan with two passes per part,
NaN records, an empty region, a chunk of one entry.

    DDPM3D_LIB=<the trusted build> python tests/test_gpu_records.py --record      # writes the golden

Arrays of more than a few hundred values (the SSIM map, the bound's workspace) enter the golden as the SHA-256 of
their bytes.
"""

import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from guided_diffusion import _hip as H
from guided_diffusion import metrics
from guided_diffusion import script_util as su
from guided_diffusion import synth

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "moment_records.npz")
VOXELS = {"wide264": 269316,            # 264 parts on the 16-byte path; threads 0..7 of the fold take two records
          "narrow": 269315,             # not a multiple of 4: the scalar path
          "capped": 2050 * 1024 + 8}    # 2051 passes: the 2048-part cap applies and a part takes two passes
VB_VOXELS, VB_T = 269315, 10
ROI_SHAPE = (64, 144, 144)
ROI_COUNTS = [1100000, 4097, 1, 0]      # 269 chunks (the fold passes 256); a second chunk of one entry; one voxel; empty
SSIM_SHAPES = {"small": (27, 33, 45), "fold320": (90, 138, 266)}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    """the integer bit patterns of a float array"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def workspace(nbytes):
    assert nbytes > 0
    return torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------ the entries
@functools.lru_cache(maxsize=None)
def moment_inputs(voxels):
    est, prev = synth.synth_noise((2, voxels), 2, seed=31)
    target = synth.synth_low_res((2, voxels), seed=32)
    u = synth.synth_low_res((2, voxels), seed=33)
    return dict(est=est, prev=prev, target=target, u=u)


def error_moments(est, target, mask, std):
    lib = H.load()
    B, voxels = est.shape
    need = lib.ddpm3d_error_moments_workspace_bytes(B, voxels)
    ws = workspace(need)
    out = torch.full((B, H.EM_REC), float("nan"), dtype=torch.float64, device="cuda")
    H.check(lib.ddpm3d_error_moments(H.ptr(est), H.ptr(target), H.ptr(mask), H.ptr(std), B, voxels, H.ptr(ws), need,
                                     H.ptr(out), H.stream()))
    return out.cpu().numpy()


def case_error_moments(size, optional):
    """-> the (2, EM_REC) records, and row 1 from a call on estimate 1 alone"""
    i = moment_inputs(VOXELS[size])
    est, target = dev(i["est"]), dev(i["target"][0])
    mask = dev((i["u"][0] > 0.25).astype(np.uint8)) if optional else None
    std = dev(np.float32(0.75) * i["u"][1]) if optional else None      # |e| <= std and <= 2 std both happen
    return {"records": error_moments(est, target, mask, std), "alone": error_moments(est[1:], target, mask, std)}


def trace_moments(est, prev, target, weight):
    lib = H.load()
    B, voxels = est.shape
    need = lib.ddpm3d_trace_moments_workspace_bytes(B, voxels)
    ws = workspace(need)
    out = torch.full((B, H.TR_REC), float("nan"), dtype=torch.float64, device="cuda")
    stride = lambda t: 0 if t is None else voxels
    H.check(lib.ddpm3d_trace_moments(H.ptr(est), H.ptr(prev), H.ptr(target), H.ptr(weight), B, voxels, stride(target),
                                     stride(weight), H.ptr(ws), need, H.ptr(out), H.stream()))
    return out.cpu().numpy()


def case_trace_moments(size, optional):
    i = moment_inputs(VOXELS[size])
    est = i["est"]
    prev = target = weight = None
    if optional:
        weight = np.where(i["u"] < 0.25, np.float32(0.0), i["u"]).astype(np.float32)
        est = est.copy()
        for b in range(2):
            at = np.flatnonzero(weight[b] == 0)[[0, -1]]
            est[b, at] = np.nan                                        # behind a zero weight: never added
        prev, target = dev(i["prev"]), dev(i["target"])
    est, weight = dev(est), dev(weight)
    one = lambda t: None if t is None else t[1:]
    return {"records": trace_moments(est, prev, target, weight),
            "alone": trace_moments(est[1:], one(prev), one(target), one(weight))}


@functools.lru_cache(maxsize=1)
def vb_inputs():
    shape = (3, 1, VB_VOXELS)
    xs = synth.synth_x_start(shape, seed=21)
    noise = synth.synth_noise(shape, 1, seed=22)[0]
    xt = (np.float32(0.8) * xs + np.float32(0.6) * noise).astype(np.float32)
    return dev(xs), dev(noise), dev(xt), dev(np.array([0, 5, VB_T], dtype=np.int64))   # the last t is out of range


def vb_tables(learn):
    d = su.create_gaussian_diffusion(steps=1000, learn_sigma=learn, timestep_respacing=str(VB_T))
    assert d.num_timesteps == VB_T
    return dev(d.coef_table()), dev(d.qcoef_table())


def case_vb_terms(learn, with_noise):
    """-> vb, xstart_mse (and mse) [3] fp32, and the digest of the 3 x parts x 4 fp64 workspace records"""
    lib = H.load()
    xs, noise, xt, t = vb_inputs()
    coef, qcoef = vb_tables(learn)
    mo = dev(synth.synth_model_output((3, 1, VB_VOXELS), learn, seed=23))
    need = lib.ddpm3d_vb_terms_workspace_bytes(3, VB_VOXELS)
    ws = workspace(need)
    vb, xm, mse = (torch.full((3,), float("nan"), device="cuda") for _ in range(3))
    flags = (H.F_LEARN_SIGMA if learn else 0) | H.F_CLIP
    H.check(lib.ddpm3d_vb_terms(H.ptr(mo), H.ptr(xs), H.ptr(xt), H.ptr(noise if with_noise else None), H.ptr(coef),
                                H.ptr(qcoef), H.ptr(t), 3, VB_VOXELS, VB_T, flags, H.ptr(ws), need, H.ptr(vb),
                                H.ptr(xm), H.ptr(mse if with_noise else None), 1, None, H.stream()))
    res = {"vb": vb.cpu().numpy(), "xstart_mse": xm.cpu().numpy(), "workspace": digest(ws.cpu().numpy())}
    if with_noise:
        res["mse"] = mse.cpu().numpy()
    assert np.isnan(res["vb"][2]) and np.isfinite(res["vb"][:2]).all()
    return res


def case_prior_bpd():
    lib = H.load()
    xs = vb_inputs()[0]
    qcoef = vb_tables(True)[1]
    need = lib.ddpm3d_vb_terms_workspace_bytes(3, VB_VOXELS)
    ws = workspace(need)
    out = torch.full((3,), float("nan"), device="cuda")
    H.check(lib.ddpm3d_prior_bpd(H.ptr(xs), H.ptr(qcoef), 3, VB_VOXELS, VB_T, H.ptr(ws), need, H.ptr(out),
                                 H.stream()))
    return {"prior_bpd": out.cpu().numpy(), "workspace": digest(ws.cpu().numpy())}


@functools.lru_cache(maxsize=1)
def roi_inputs():
    voxels = int(np.prod(ROI_SHAPE))
    picked = np.random.default_rng(34).permutation(voxels)[:sum(ROI_COUNTS)]
    ends = np.cumsum(ROI_COUNTS)
    index = np.concatenate([np.sort(picked[e - n:e]) for n, e in zip(ROI_COUNTS, ends)]).astype(np.int64)
    ix = metrics.RoiIndex(ROI_SHAPE, range(1, len(ROI_COUNTS) + 1), ROI_COUNTS, dev(index))
    est = synth.synth_noise((2,) + ROI_SHAPE, 1, seed=35)[0]
    target = synth.synth_low_res(ROI_SHAPE, seed=36)
    return ix, dev(est), dev(target)


def case_roi_moments(with_target):
    lib = H.load()
    ix, est, target = roi_inputs()
    need = lib.ddpm3d_roi_moments_workspace_bytes(2, ix.desc)
    assert need == 2 * (269 + 2 + 1) * H.ROI_REC * 8
    ws = workspace(need)
    out = torch.full((2, len(ix), H.ROI_REC), float("nan"), dtype=torch.float64, device="cuda")
    H.check(lib.ddpm3d_roi_moments(H.ptr(est), H.ptr(target if with_target else None), 2, ix.voxels, ix.desc,
                                   H.ptr(ws), need, H.ptr(out), H.stream()))
    rec = out.cpu().numpy()
    assert rec[:, :, H.ROI_N].tolist() == [ROI_COUNTS] * 2
    assert (rec[:, 3, H.ROI_MIN_X] == np.inf).all() and (rec[:, 3, H.ROI_MAX_X] == -np.inf).all()
    return {"records": rec}


@functools.lru_cache(maxsize=None)
def ssim_inputs(size):
    shape = SSIM_SHAPES[size]
    target = synth.synth_low_res(shape, seed=37)
    est = (target[None] + np.float32(0.1) * synth.synth_noise((2,) + shape, 1, seed=38)[0]).astype(np.float32)
    mask = (synth.synth_low_res(shape, seed=39) > 0.2).astype(np.uint8) if size == "small" else None
    return dev(est), dev(target), dev(mask)


C1, C2 = 0.01 ** 2, 0.03 ** 2            # data_range 1


def case_ssim3d(size):
    lib = H.load()
    est, target, mask = ssim_inputs(size)
    D, Hh, W = SSIM_SHAPES[size]
    need = lib.ddpm3d_ssim3d_workspace_bytes(2, D, Hh, W)
    if size == "fold320":                # 8 x 8 tiles x 5 chunks of {sum, count} per estimate: the fold passes 256
        assert need == 2 * 320 * 2 * 8
    ws = workspace(need)
    out = torch.full((2, 2), float("nan"), dtype=torch.float64, device="cuda")
    smap = torch.full((2, D - 10, Hh - 10, W - 10), float("nan"), device="cuda")
    H.check(lib.ddpm3d_ssim3d(H.ptr(est), H.ptr(target), H.ptr(mask), 2, D, Hh, W, C1, C2, H.ptr(ws), need,
                              H.ptr(smap), H.ptr(out), H.stream()))
    return {"records": out.cpu().numpy(), "map": digest(smap.cpu().numpy())}


def case_msssim3d(size):
    lib = H.load()
    est, target, mask = ssim_inputs(size)
    D, Hh, W = SSIM_SHAPES[size]
    need = lib.ddpm3d_msssim3d_workspace_bytes(2, D, Hh, W, 2)
    ws = workspace(need)
    out = torch.full((2, 2, 3), float("nan"), dtype=torch.float64, device="cuda")
    H.check(lib.ddpm3d_msssim3d(H.ptr(est), H.ptr(target), H.ptr(mask), 2, D, Hh, W, 2, C1, C2, H.ptr(ws), need,
                                H.ptr(out), H.stream()))
    return {"records": out.cpu().numpy()}


CASES = {}
for _size in VOXELS:
    for _opt in (False, True):
        _tag = "%s/%s" % (_size, "all" if _opt else "bare")
        CASES["error_moments/" + _tag] = functools.partial(case_error_moments, _size, _opt)
        CASES["trace_moments/" + _tag] = functools.partial(case_trace_moments, _size, _opt)
for _learn in (True, False):
    for _noise in (True, False):
        CASES["vb_terms/%s/%s" % ("learned" if _learn else "fixed", "noise" if _noise else "bare")] = \
            functools.partial(case_vb_terms, _learn, _noise)
CASES["prior_bpd"] = case_prior_bpd
CASES["roi_moments/target"] = functools.partial(case_roi_moments, True)
CASES["roi_moments/bare"] = functools.partial(case_roi_moments, False)
for _size in SSIM_SHAPES:
    CASES["ssim3d/" + _size] = functools.partial(case_ssim3d, _size)
    CASES["msssim3d/" + _size] = functools.partial(case_msssim3d, _size)


def run(case):
    """-> {key: integer bit patterns}, after the checks that need no golden"""
    res = CASES[case]()
    torch.cuda.synchronize()
    alone = res.pop("alone", None)
    if alone is not None:                # row 1 of the batch carries the bits of the call on estimate 1
        assert np.array_equal(bits(alone[0]), bits(res["records"][1])), case
    return {k: (v if v.dtype == np.uint8 else bits(v)) for k, v in res.items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bits_are_the_recorded_ones(golden, case):
    g = golden("moment_records.npz")
    got = run(case)
    want = {k.rsplit("/", 1)[1]: g[k] for k in g.files if k.rsplit("/", 1)[0] == case}
    assert sorted(got) == sorted(want), case
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (case, k)
        assert np.array_equal(got[k], want[k]), (case, k, got[k], want[k])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: DDPM3D_LIB=<the trusted build> python tests/test_gpu_records.py --record")
    out = {}
    for name in sorted(CASES):
        for k, v in run(name).items():
            out["%s/%s" % (name, k)] = v
    np.savez(GOLDEN_FILE, **out)
    print("wrote %s from %s: %d arrays, %d bytes" % (GOLDEN_FILE, H.LIB_PATH, len(out), os.path.getsize(GOLDEN_FILE)))
