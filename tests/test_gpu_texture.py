"""
GPU tier of the per-region texture figures: ddpm3d_roi_texture's co-occurrence matrices, histograms
and side counters against the numpy restatement of tests/texture_ref.py, exactly (they are integers), on a 5 x 6 x 7
volume (one region touching all six faces, two regions sharing a face, a one-voxel region; NaN and infinite voxels,
values below the first and above the last bin; 2, 8 and 64 levels; B = 1 and 3 with their own lo and inv_w per
estimate and region), across chunk borders (17 x 16 x 16: two chunks; 40 x 32 x 32: ten), an empty region through
the C entry, repeatability over sentinel-filled outputs, every refusal of the C entry, texture_figures against the
restatement's figures under the summation bound, the two discretisation modes, one device-to-host copy per call,
roi_report's texture blocks, and the inference script's --roi_texture_bin.
"""

import ctypes
import importlib.util
import json
import os
import warnings

import numpy as np
import pytest
import torch

import texture_ref as T
from conftest import PKG
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

SHAPE = (5, 6, 7)                                                  # W is no multiple of 4
SENTINEL = 0x5A5A5A5A5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _labels(kind, shape=SHAPE):
    lab = np.ones(shape, dtype=np.int32)
    if kind == "two":                                             # two regions sharing a face
        lab[:, :, 4:] = 2
    elif kind == "voxel":                                         # a box, a gap, and a one-voxel region in the corner
        lab[:] = 0
        lab[1:4, 1:5, 0:5] = 4
        lab[4, 5, 6] = 9
    return lab


def _volumes(shape=SHAPE, n=3, seed=5):
    """n volumes in about [-0.2, 1.3] with a NaN, a +inf and a -inf voxel each, at places of their own"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.3, size=(n,) + shape).astype(np.float32)
    flat = x.reshape(n, -1)
    for b in range(n):
        at = rng.choice(flat.shape[1], size=4, replace=False)
        flat[b, at[:2]] = np.nan
        flat[b, at[2]], flat[b, at[3]] = np.inf, -np.inf
    return x


def _entry(est, index, region_of, lo, inv_w, levels, fill=SENTINEL, desc=None, regions=None):
    """one call of the C entry over sentinel-filled outputs -> (glcm, hist, counts) as numpy int64"""
    est = est if est.dim() == 4 else est[None]
    K, R = est.shape[0], len(index) if regions is None else regions
    D, H, W = est.shape[1:]
    out = [torch.full(s, fill, dtype=torch.int64, device="cuda")
           for s in ((K, R, levels, levels), (K, R, levels), (K, R, _hip.TEX_REC))]
    _hip.check(_hip.load().ddpm3d_roi_texture(
        _hip.ptr(est), K, D, H, W, index.desc if desc is None else desc, _hip.ptr(region_of), _hip.ptr(lo),
        _hip.ptr(inv_w), levels, _hip.ptr(out[0]), _hip.ptr(out[1]), _hip.ptr(out[2]), _hip.stream()))
    return [o.cpu().numpy() for o in out]


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("glcm", "hist", "counts")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


# ------------------------------------------------------------------------------------------ exact equality
@pytest.mark.parametrize("levels", [2, 8, 64])
@pytest.mark.parametrize("kind", ["all", "two", "voxel"])
def test_matrices_equal_the_restatement_exactly(kind, levels):
    lab = _labels(kind)
    x = _volumes()
    index = metrics.roi_index(dev(lab))
    R = len(index)
    rng = np.random.default_rng(levels)
    lo = rng.uniform(-0.1, 0.2, size=(3, R)).astype(np.float32)           # values below lo ...
    inv_w = (levels / rng.uniform(0.7, 1.0, size=(3, R))).astype(np.float32)   # ... and above the top bin
    want = T.roi_texture(x, lab, lo, inv_w, levels)
    assert (want[2][:, 0, T.BELOW] > 0).all() and (want[2][:, 0, T.ABOVE] > 0).all()
    n_region = np.array(index.counts)
    assert (want[2][:, :, T.N] == n_region - [[(np.isnan(x[b]) & (lab == v)).sum() for v in index.labels]
                                              for b in range(3)]).all()
    region_of = index.region_of()
    assert region_of.dtype == torch.int16 and tuple(region_of.shape) == SHAPE and index.region_of() is region_of
    ordinal = np.zeros(SHAPE, dtype=np.int16)
    for r, v in enumerate(index.labels):
        ordinal[lab == v] = r + 1
    assert np.array_equal(region_of.cpu().numpy(), ordinal)
    got = _entry(dev(x), index, region_of, dev(lo), dev(inv_w), levels)
    _same(got, want, "B = 3")
    assert np.array_equal(got[0], got[0].transpose(0, 1, 3, 2))
    assert (got[0].sum(axis=(2, 3)) == 2 * got[2][:, :, T.PAIRS]).all() and (got[1].sum(axis=2) == got[2][:, :, 0]).all()
    for b in range(3):                                                   # B = 1: row b of the stack
        single = _entry(dev(x[b]), index, region_of, dev(lo[b:b + 1]), dev(inv_w[b:b + 1]), levels)
        _same(single, [g[b:b + 1] for g in got], "B = 1, estimate %d" % b)
    if kind == "voxel":
        assert got[2][:, 1, T.PAIRS].tolist() == [0, 0, 0] and (got[0][:, 1] == 0).all()


def test_a_constant_box_and_a_flat_region():
    """the closed form of the CPU tier through the kernel, and inv_w = 0"""
    index = metrics.roi_index(dev(_labels("all")))
    x = dev(np.full(SHAPE, 0.52, dtype=np.float32))
    one = lambda v: torch.full((1, 1), v, device="cuda")
    glcm, hist, counts = _entry(x, index, index.region_of(), one(0.0), one(20.0), 64)
    assert glcm[0, 0, 10, 10] == 3742 and glcm.sum() == 3742 and hist[0, 0, 10] == 210
    assert counts[0, 0].tolist() == [210, 0, 0, 1871]
    glcm, hist, counts = _entry(x, index, index.region_of(), one(0.52), one(0.0), 2)
    assert glcm[0, 0].tolist() == [[3742, 0], [0, 0]] and counts[0, 0].tolist() == [210, 0, 0, 1871]


@pytest.mark.parametrize("shape", [(17, 16, 16), (40, 32, 32)], ids=["two-chunks", "ten-chunks"])
def test_pairs_across_chunk_borders(shape):
    """one region of 4352 entries (two chunks) and of 40960 (ten: more than one workgroup whatever span it keeps)"""
    lab = np.ones(shape, dtype=np.int32)
    x = np.random.default_rng(9).uniform(0.0, 1.0, size=(2,) + shape).astype(np.float32)
    index = metrics.roi_index(dev(lab))
    assert index.counts == [int(np.prod(shape))] and index.counts[0] > _hip.ROI_CHUNK
    lo = np.zeros((2, 1), dtype=np.float32)
    inv_w = np.full((2, 1), 16.0, dtype=np.float32)
    got = _entry(dev(x), index, index.region_of(), dev(lo), dev(inv_w), 16)
    _same(got, T.roi_texture(x, lab, lo, inv_w, 16))
    D, H, W = shape
    assert got[2][0, 0, T.PAIRS] == sum((D - abs(a)) * (H - abs(b)) * (W - abs(c)) for a, b, c in T.DIRECTIONS)


def test_an_empty_region_through_the_c_entry():
    """offsets by hand: regions of 5, 0, 205 and 0 entries of the whole volume's list"""
    lab = _labels("all")
    x = _volumes(n=2)
    index = metrics.roi_index(dev(lab))
    offsets, chunks = [0, 5, 5, 210, 210], [0, 1, 1, 2, 2]
    host = (ctypes.c_int64 * 5)(*offsets)
    tab = torch.tensor([offsets, chunks], dtype=torch.int64).cuda()
    desc = _hip.RoiIndex(4, 210, host, _hip.ptr(tab[0]), _hip.ptr(tab[1]), _hip.ptr(index.index))
    mine = np.full(210, 3, dtype=np.int32)
    mine[:5] = 1
    mine = mine.reshape(SHAPE)
    lo = np.zeros((2, 4), dtype=np.float32)
    inv_w = np.full((2, 4), 8.0, dtype=np.float32)
    got = _entry(dev(x), index, dev(mine.astype(np.int16)), dev(lo), dev(inv_w), 8, desc=desc, regions=4)
    _same(got, T.roi_texture(x, mine, lo, inv_w, 8, found=[1, 2, 3, 4]))
    for g in got:
        assert (g[:, 1] == 0).all() and (g[:, 3] == 0).all() and (g[:, 2] != 0).any()


def test_region_of_decides_the_neighbours_and_no_load_leaves_the_volume():
    """a region_of that claims every voxel for region 1 while the index lists only the box: the pairs from the box's
    voxels to every neighbour inside the volume count, none beyond a face or across a row end"""
    lab = _labels("voxel")
    lab[lab == 9] = 0
    x = np.random.default_rng(2).uniform(0.0, 1.0, size=SHAPE).astype(np.float32)
    index = metrics.roi_index(dev(lab))
    everywhere = torch.ones(SHAPE, dtype=torch.int16, device="cuda")
    one = lambda v: torch.full((1, 1), v, device="cuda")
    got = _entry(dev(x), index, everywhere, one(0.0), one(8.0), 8)
    box = lab == 4
    pairs = 0
    for d in T.DIRECTIONS:
        a, b = zip(*[T._pair(n, dd) for n, dd in zip(SHAPE, d)])
        pairs += int(box[a].sum())                                       # the lower voxel is the index's
    assert got[2][0, 0].tolist() == [60, 0, 0, pairs]


# ------------------------------------------------------------------------------------------ repeatability
def test_two_runs_over_sentinels_give_the_same_bytes():
    lab, x = _labels("two"), _volumes()
    index = metrics.roi_index(dev(lab))
    lo = dev(np.zeros((3, 2), dtype=np.float32))
    inv_w = dev(np.full((3, 2), 64.0, dtype=np.float32))
    first = _entry(dev(x), index, index.region_of(), lo, inv_w, 64, fill=SENTINEL)
    second = _entry(dev(x), index, index.region_of(), lo, inv_w, 64, fill=-1)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    _same(first, T.roi_texture(x, lab, 0.0, 64.0, 64))


# ------------------------------------------------------------------------------------------ refusals
def test_the_c_entry_refuses_before_any_launch():
    lab = _labels("two")
    index = metrics.roi_index(dev(lab))
    lib = _hip.load()
    x = dev(_volumes(n=1))
    region_of = index.region_of()
    lo, inv_w = torch.zeros((1, 2), device="cuda"), torch.ones((1, 2), device="cuda")
    outs = [torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda") for n in (2 * 64 * 64, 2 * 64, 2 * 4)]
    good = dict(est=_hip.ptr(x), B=1, D=5, H=6, W=7, index=index.desc, region_of=_hip.ptr(region_of), lo=_hip.ptr(lo),
                inv_w=_hip.ptr(inv_w), levels=8, glcm=_hip.ptr(outs[0]), hist=_hip.ptr(outs[1]),
                counts=_hip.ptr(outs[2]))

    def desc(regions=2, entries=210, offsets=(0, 120, 210), null=None):
        host = (ctypes.c_int64 * len(offsets))(*offsets)
        p = dict(offsets=host, d_offsets=index.desc.d_offsets, d_chunks=index.desc.d_chunks,
                 d_index=index.desc.d_index)
        if null:
            p[null] = None
        d = _hip.RoiIndex(regions, entries, p["offsets"], p["d_offsets"], p["d_chunks"], p["d_index"])
        d._keep = host
        return d

    assert index.offsets == [0, 120, 210]
    bad = [dict(**{k: None}) for k in ("est", "region_of", "lo", "inv_w", "glcm", "hist", "counts", "index")]
    bad += [dict(index=desc(null=k)) for k in ("offsets", "d_offsets", "d_chunks", "d_index")]
    bad += [dict(B=0), dict(B=_hip.MAX_DRAWS + 1), dict(D=0), dict(H=0), dict(W=0), dict(D=65536), dict(H=65536),
            dict(W=65536), dict(D=2048, H=2048, W=512), dict(levels=1), dict(levels=65), dict(levels=-3)]
    bad += [dict(index=desc(regions=0)), dict(index=desc(regions=_hip.ROI_MAX_REGIONS + 1)),
            dict(index=desc(entries=-1)), dict(index=desc(offsets=(1, 120, 210))),
            dict(index=desc(offsets=(0, 211, 210))), dict(index=desc(offsets=(0, 120, 100))),
            dict(index=desc(offsets=(0, 120, 200)))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.ddpm3d_roi_texture(a["est"], a["B"], a["D"], a["H"], a["W"], a["index"], a["region_of"], a["lo"],
                                    a["inv_w"], a["levels"], a["glcm"], a["hist"], a["counts"], _hip.stream())
        assert rc == _hip.E_INVAL, change
        assert lib.ddpm3d_last_error().decode().startswith("roi_texture:"), (change, lib.ddpm3d_last_error())
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    a = good                                                             # and the same arguments untouched do run
    _hip.check(lib.ddpm3d_roi_texture(a["est"], a["B"], a["D"], a["H"], a["W"], a["index"], a["region_of"], a["lo"],
                                      a["inv_w"], a["levels"], a["glcm"], a["hist"], a["counts"], _hip.stream()))
    assert int(outs[2][0]) == 120 - int(np.isnan(x.cpu().numpy()[0][lab == 1]).sum())


def test_python_arguments_that_do_not_fit_the_index_are_refused():
    index = metrics.roi_index(dev(_labels("two")))
    x = torch.zeros(SHAPE, device="cuda")
    with pytest.raises(ValueError, match="roi_texture: estimate"):
        metrics.roi_texture(x[:, :, :6].contiguous(), index, bin_width=0.1)
    with pytest.raises(ValueError, match="estimates"):
        metrics.roi_texture(torch.zeros((65,) + SHAPE, device="cuda"), index, bin_width=0.1)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.roi_texture(x.cpu(), index, bin_width=0.1)


# ------------------------------------------------------------------------------------------ figures and modes
@pytest.fixture(scope="module")
def phantom():
    """the CPU tier's phantom with two more regions, its index and three 'draws': built once, never changed"""
    clean, noisy, lab = T.phantom()
    lab[0:4, 0:6, 0:6] = 2
    lab[20:24, 30:40, 33:40] = 7
    rng = np.random.default_rng(11)
    draws = np.stack([clean + 0.03 * rng.standard_normal(clean.shape) for _ in range(3)]).astype(np.float32)
    return clean, noisy, lab, draws, metrics.roi_index(dev(lab))


@pytest.mark.parametrize("levels", [64, 8])
def test_figures_match_the_restatement_under_the_summation_bound(phantom, levels):
    """both sides run fp64 arithmetic on identical integers; only the summation order differs:
    |figure - restatement| <= (levels^2 + 2) 2^-53 sum |terms|"""
    clean, noisy, lab, draws, index = phantom
    stack = np.stack([clean, noisy])
    width = 0.05 * 64 / levels
    res = metrics.roi_texture(dev(stack), index, levels=levels, bin_width=width)
    assert res.glcm.shape == (2, 3, levels, levels) and res.levels == levels and res.batched
    assert (res.lo == 0).all() and (res.inv_w == np.float32(1.0 / width)).all()
    _same((res.glcm, res.hist, res.counts), T.roi_texture(stack, lab, res.lo, res.inv_w, levels))
    got = metrics.texture_figures(res)
    worst = 0.0
    for b in range(2):
        for r in range(3):
            want, mag = T.figures(res.glcm[b, r], res.hist[b, r], res.counts[b, r], res.lo[b, r], res.inv_w[b, r])
            assert set(got[b][r]) == set(want)
            for k, w in want.items():
                g = got[b][r][k]
                if w is None or isinstance(w, int):
                    assert g == w, (b, r, k)
                    continue
                bound = (levels ** 2 + 2) * 2.0 ** -53 * mag[k]
                worst = max(worst, abs(g - w) / bound if bound else 0.0)
                assert abs(g - w) <= bound, (b, r, k, g, w, bound)
    print("levels %d: largest deviation %.3g of its bound" % (levels, worst))
    if levels == 64:                                                     # the figures of the feature's motivation
        assert got[1][0]["contrast"] > 10 * got[0][0]["contrast"] and got[0][0]["clamped"] == 0
    single = metrics.roi_texture(dev(noisy), index, levels=levels, bin_width=width)
    assert not single.batched and metrics.texture_figures(single) == got[1]


def test_fixed_bin_number_spans_the_region_and_clamps_nothing(phantom):
    clean, noisy, lab, draws, index = phantom
    flat = noisy.copy()
    flat[lab == 7] = 0.75                                                # a flat region: inv_w = 0
    stack = np.stack([clean, flat])
    for levels in (64, 5):
        res = metrics.roi_texture(dev(stack), index, levels=levels)
        for b in range(2):
            for r, v in enumerate(index.labels):
                mn, mx = stack[b][lab == v].min(), stack[b][lab == v].max()
                assert res.lo[b, r] == mn
                if mx > mn:
                    assert res.inv_w[b, r] == pytest.approx(levels / (float(mx) - float(mn)), rel=1e-6)
                    assert res.inv_w[b, r] < levels / (float(mx) - float(mn))
                    assert res.hist[b, r, 0] > 0 and res.hist[b, r, levels - 1] > 0
                else:
                    assert res.inv_w[b, r] == 0 and res.hist[b, r, 0] == res.counts[b, r, T.N]
        assert (res.counts[:, :, T.BELOW] == 0).all() and (res.counts[:, :, T.ABOVE] == 0).all()
        assert (res.counts[:, :, T.N] == np.array(index.counts)).all()
        _same((res.glcm, res.hist, res.counts), T.roi_texture(stack, lab, res.lo, res.inv_w, levels))
        figs = metrics.texture_figures(res)
        assert all(f["clamped"] == 0 for row in figs for f in row)
        assert figs[1][2]["p50"] is None and figs[1][2]["joint_entropy"] == 0 and figs[1][2]["correlation"] is None


@pytest.mark.parametrize("mode", ["fixed-size", "fixed-number"])
def test_one_device_to_host_copy_per_call(phantom, mode):
    """under torch's sync debug mode every blocking call warns: roi_texture makes one, the copy of its buffer"""
    clean, noisy, lab, draws, index = phantom
    x = dev(draws)
    kw = dict(bin_width=0.05) if mode == "fixed-size" else {}
    metrics.roi_texture(x, index, **kw)                                   # the library is loaded, region_of is built
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            metrics.roi_texture(x, index, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    blocking = [w for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(blocking) == 1, [str(w.message) for w in seen]


# ------------------------------------------------------------------------------------------ the report
TEXTURE_KEYS = {"texture", "texture_rel", "draw_texture", "texture_std"}


def test_report_carries_the_texture_of_target_estimate_and_draws(phantom):
    clean, noisy, lab, draws, index = phantom
    mean = draws.mean(axis=0, dtype=np.float64).astype(np.float32)
    request = {"bin_width": 0.05, "levels": 32, "lower": 0.25}
    got = metrics.roi_report(dev(mean), dev(clean), index, draws=dev(draws), texture=request)
    plain = metrics.roi_report(dev(mean), dev(clean), index, draws=dev(draws), texture=None)
    assert plain == metrics.roi_report(dev(mean), dev(clean), index, draws=dev(draws))
    assert not any(k in plain[v][w] for v in plain for w in ("target", "estimate") for k in TEXTURE_KEYS)
    stripped = {v: {"n": r["n"], "target": {k: x for k, x in r["target"].items() if k not in TEXTURE_KEYS},
                    "estimate": {k: x for k, x in r["estimate"].items() if k not in TEXTURE_KEYS}}
                for v, r in got.items()}
    assert stripped == plain                                             # without texture: today's dict
    fig = lambda vol: metrics.texture_figures(metrics.roi_texture(dev(vol), index, **request))
    want_t, want_e, want_d = fig(clean), fig(mean), [fig(d) for d in draws]
    assert want_d == fig(draws)                                          # the stack: K lists of R dicts
    for r, v in enumerate(index.labels):
        t, e = got[v]["target"], got[v]["estimate"]
        assert set(t) & TEXTURE_KEYS == {"texture"} and set(e) & TEXTURE_KEYS == TEXTURE_KEYS
        assert t["texture"] == want_t[r] and e["texture"] == want_e[r]
        assert e["draw_texture"] == [d[r] for d in want_d]
        for k in ("n", "pairs") + metrics.TEXTURE_FIGURES:
            a, b = want_e[r][k], want_t[r][k]
            rel = None if a is None or b is None or b == 0 else (a - b) / b
            assert e["texture_rel"][k] == rel, (v, k)
            vals = [d[r][k] for d in want_d if d[r][k] is not None]
            if len(vals) < 2:
                assert e["texture_std"][k] is None
            else:
                assert e["texture_std"][k] == pytest.approx(np.std(vals, ddof=1), rel=1e-12, abs=1e-300), (v, k)
        assert e["texture_std"]["contrast"] > 0 and e["texture_rel"]["n"] == 0
    by_records = metrics.roi_report(dev(mean), dev(clean), index, draws=[metrics.roi_moments(dev(d), index) for d in draws],
                                    texture=request, draw_texture=want_d, target_texture=want_t)
    assert by_records == got                                             # draws as records: the same report


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()


def _script():
    spec = importlib.util.spec_from_file_location("ddpm3d_infer_entry", os.path.join(PKG, "scripts", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_writes_the_texture_of_every_row(tmp_path, capsys):
    import metrics_ref
    target = metrics_ref.phantom((20, 40, 40), seed=4)                      # (D, H, W): 3 x 3 x 2 patches of 16^3
    low = metrics_ref.noisy(target, 0.1, seed=4)
    np.savez(tmp_path / "pet.npz", low)
    np.savez(tmp_path / "full.npz", target)
    mod = _script()
    common = FLAGS + ["--base_samples", str(tmp_path / "pet.npz"), "--target_samples", str(tmp_path / "full.npz")]
    with pytest.raises(SystemExit):                                        # a two-flag refusal, through main
        mod.main(common + ["--save_dir", str(tmp_path / "no"), "--roi_texture_bin", "0.05"])
    assert "--roi_texture_bin needs regions" in capsys.readouterr().err
    path = mod.main(common + ["--save_dir", str(tmp_path / "tex"), "--roi_threshold", repr(0.4 * float(target.max())),
                              "--roi_connectivity", "6", "--roi_texture_bin", "0.05", "--voxel_spacing", "3.27", "2.0",
                              "1.5", "--baseline_gaussian_fwhm", "5"])
    rep = json.load(open(tmp_path / "tex" / "metrics_pet.json"))
    roi = rep["roi"]
    assert roi["texture"] == {"bin_width": 0.05, "levels": 64, "lower": 0.0, "directions": 13}
    labels = np.load(roi["labels"])["arr_0"].transpose(1, 2, 0)             # (D, H, W) -> (H, W, Z), as scored
    keep = np.ones(labels.shape, dtype=np.uint8)                            # Hann weight 0: the outermost planes
    keep[[0, -1]] = 0
    keep[:, [0, -1]] = 0
    keep[:, :, [0, -1]] = 0
    index = metrics.roi_index(dev(labels), keep=dev(keep))
    assert [str(v) for v in index.labels] == list(roi["regions"]) and len(index) >= 1
    tgt = dev(target.transpose(1, 2, 0))
    want = metrics.texture_figures(metrics.roi_texture(tgt, index, bin_width=0.05))
    want_den = metrics.texture_figures(metrics.roi_texture(dev(np.load(path)["arr_0"]), index, bin_width=0.05))
    keys = {"n", "pairs"} | set(metrics.TEXTURE_FIGURES)
    for r, v in enumerate(index.labels):
        row = roi["regions"][str(v)]
        assert list(row) == ["n", "target", "input", "gaussian", "denoised"]
        assert row["target"]["texture"] == want[r] and "texture_rel" not in row["target"]
        assert row["denoised"]["texture"] == want_den[r]
        for name in ("input", "gaussian", "denoised"):
            assert set(row[name]["texture"]) == set(row[name]["texture_rel"]) == keys
            assert "draw_texture" not in row[name]
    big = max(roi["regions"].values(), key=lambda r: r["n"])
    assert big["gaussian"]["texture"]["contrast"] < big["input"]["texture"]["contrast"]
    log = open(tmp_path / "tex" / "log.txt").read()
    assert "; contrast " in log and "; joint_entropy " in log
