"""
GPU tier of the radial spectra and the Fourier shell correlation: ddpm3d_dft3 coefficient by
coefficient against numpy.fft under the derived rounding bound (2 x 2 x 2, 5 x 6 x 7, 9 x 33 x 34 and 33 x 18 x 65:
odd and even W, M, N and K across one 32- and one 64-tile border, odd K), plane-wave known answers, ddpm3d_shell_sums
on numpy-made spectra (exact counts, a shell over three chunks, an empty shell), the driver against its two parts bit
for bit, Parseval, estimate == target, batch independence and NaN containment, repeatability over sentinel-filled
buffers, every refusal of the three C entries, the one device-to-host copy of metrics.shell_spectrum, the three single
passes of the timing entry against the transform, the README's phantom, and the inference script's --spectrum on the
one-shot path, the joint path and with --num_draws.
"""

import ctypes
import warnings

import numpy as np
import pytest
import torch

import spectrum_ref as R
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 2), (5, 6, 7), (9, 33, 34), (33, 18, 65)]
SPACING = (3.27, 2.0, 1.5)
U = 2.0 ** -24
SENTINEL = -7.25e30


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bound(shape, wv):
    """|coefficient - exact| <= 1.01 c 2^-24 sum |w (v - p)|, c = (W + 2) + (2H + 2) + (2D + 2)"""
    D, H, W = shape
    return 1.01 * ((W + 2) + (2 * H + 2) + (2 * D + 2)) * U * np.abs(wv).sum()


def _volumes(shape, n, offset, seed=0):
    rng = np.random.default_rng(seed + 17 * int(offset))
    return (offset + 0.1 * rng.normal(size=(n,) + shape)).astype(np.float32)


def _weighted(v, window, p):
    """w (v - p) in fp64 with v - p formed in fp32, per volume of the stack"""
    d = (v - np.asarray(p, dtype=np.float32).reshape(-1, 1, 1, 1)).astype(np.float64)
    return R.weight(window, v.shape[1:])[None] * d


def _dft3(v, plan, pivot=None):
    re, im = metrics.dft3(dev(v), plan, None if pivot is None else dev(np.asarray(pivot, dtype=np.float32)))
    return re.cpu().numpy().astype(np.float64) + 1j * im.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------ the transform
@pytest.mark.parametrize("window", ["hann", "none"])
@pytest.mark.parametrize("shape", SHAPES)
def test_dft3_stays_under_the_rounding_bound(shape, window):
    plan = metrics.spectrum_plan(shape, SPACING, window=window)
    worst = 0.0
    for offset in (0.0, 4.0):
        v = _volumes(shape, 3, offset)
        for pivot in (None, v.reshape(3, -1).mean(axis=1).astype(np.float32)):
            p = np.zeros(3, dtype=np.float32) if pivot is None else pivot
            wv = _weighted(v, window, p)
            want = np.fft.rfftn(wv, axes=(1, 2, 3))
            got = _dft3(v, plan, pivot)
            assert got.shape == want.shape
            for b in range(3):
                share = np.abs(got[b] - want[b]).max() / _bound(shape, wv[b])
                worst = max(worst, share)
                assert share <= 1.0, (offset, pivot is not None, b, share)
                single = _dft3(v[b], plan, None if pivot is None else pivot[b:b + 1])       # B = 1: the same bits
                assert single.shape == want[b].shape and np.array_equal(single, got[b])
    print("dft3 %s %s: largest share of the coefficient bound %.4f" % (shape, window, worst))


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_plane_waves_land_on_their_twin_coefficients(shape):
    D, H, W = shape
    plan = metrics.spectrum_plan(shape, SPACING, window="none")
    waves = [(1, 2, 0), (D - 1, 1, 1), (2, H - 2, W // 2 - 1 if W // 2 > 1 else 1), (0, 0, 2)]
    if W % 2 == 0:
        waves.append((1, 0, W // 2))
    d, h, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    v = np.stack([np.cos(2 * np.pi * (a * d / D + b * h / H + c * x / W)) for a, b, c in waves]).astype(np.float32)
    got = _dft3(v, plan)
    V = D * H * W
    for i, (a, b, c) in enumerate(waves):
        bound = _bound(shape, v[i].astype(np.float64))
        want = np.zeros(got[i].shape)
        twin = ((-a) % D, (-b) % H)
        if c == 0 or 2 * c == W:               # both twins lie in the half spectrum (or coincide: a real wave, V)
            if twin == (a, b):
                want[a, b, c] = V
            else:
                want[a, b, c] = want[twin[0], twin[1], c] = V / 2
        else:
            want[a, b, c] = V / 2
        # the wave itself is rounded to fp32: its error enters like a volume of |error| <= 2^-24
        assert np.abs(got[i] - want).max() <= bound + V * U, (a, b, c)


# ------------------------------------------------------------------------------------------ the shell sums
def _index(shape, counts, at):
    return metrics.RoiIndex(shape, range(1, len(counts) + 1), counts, at)


def _shell_sums(x, y, dims, index, fill=SENTINEL, ws_fill=SENTINEL):
    """the C entry over sentinel-filled output and workspace -> (B, S, REC) numpy"""
    lib = _hip.load()
    B = x[0].shape[0]
    need = lib.ddpm3d_shell_sums_workspace_bytes(B, index.desc)
    assert need >= 16 and need % 16 == 0
    ws = torch.full((need // 8,), ws_fill, dtype=torch.float64, device="cuda")
    out = torch.full((B, len(index), _hip.SP_REC), fill, dtype=torch.float64, device="cuda")
    yr, yi = (None, None) if y is None else y
    _hip.check(lib.ddpm3d_shell_sums(_hip.ptr(x[0]), _hip.ptr(x[1]), _hip.ptr(yr), _hip.ptr(yi), B, *dims, index.desc,
                                     _hip.ptr(ws), need, _hip.ptr(out), _hip.stream()))
    return out.cpu().numpy()


def _sums_ref(xr, xi, yr, yi, W, members):
    """fp64 sums of one estimate over one shell's half-spectrum indices, and the sum of |term| per column"""
    Wh = W // 2 + 1
    kw = members % Wh
    w = np.where((kw > 0) & (2 * kw != W), 2.0, 1.0)
    a = xr[members].astype(np.float64) + 1j * xi[members].astype(np.float64)
    rec, mag = np.zeros(_hip.SP_REC), np.zeros(_hip.SP_REC)
    rec[_hip.SP_N] = w.sum()
    rec[_hip.SP_SUM_XX] = mag[_hip.SP_SUM_XX] = (w * np.abs(a) ** 2).sum()
    if yr is not None:
        b = yr[members].astype(np.float64) + 1j * yi[members].astype(np.float64)
        rec[_hip.SP_SUM_YY] = mag[_hip.SP_SUM_YY] = (w * np.abs(b) ** 2).sum()
        rec[_hip.SP_SUM_XY] = (w * (a * np.conj(b)).real).sum()
        mag[_hip.SP_SUM_XY] = (w * (np.abs(a.real * b.real) + np.abs(a.imag * b.imag))).sum()
        rec[_hip.SP_SUM_EE] = mag[_hip.SP_SUM_EE] = (w * np.abs(a - b) ** 2).sum()
    return rec, mag


@pytest.mark.parametrize("with_target", [True, False])
def test_shell_sums_of_numpy_spectra(with_target):
    D, H, W = 40, 32, 32
    Wh = W // 2 + 1
    coeffs = D * H * Wh                                                 # 21760: shell 0 spans three chunks, 2 four
    rng = np.random.default_rng(8)
    perm = rng.permutation(coeffs)
    cut = 2 * _hip.ROI_CHUNK + 777
    members = [np.sort(perm[:cut]), np.zeros(0, dtype=np.int64), np.sort(perm[cut:])]      # shell 1 is empty
    index = _index((D, H, Wh), [len(m) for m in members], dev(np.concatenate(members).astype(np.int64)))
    x = rng.normal(size=(2, 3, coeffs)).astype(np.float32) * 100
    y = rng.normal(size=(2, coeffs)).astype(np.float32) * 100 if with_target else None
    got = _shell_sums(dev(x), None if y is None else dev(y), (D, H, W), index)
    assert got.shape == (3, 3, _hip.SP_REC)
    full = np.bincount(np.repeat(np.arange(3), [len(m) for m in members]),
                       weights=np.where((np.concatenate(members) % Wh > 0) & (2 * (np.concatenate(members) % Wh) != W),
                                        2, 1), minlength=3)
    assert full.sum() == D * H * W
    for b in range(3):
        assert got[b, :, _hip.SP_N].tolist() == full.tolist()            # exactly the full spectrum's counts
        assert (got[b, :, 5] == 0).all() and (got[b, 1] == 0).all()       # the padding column; the empty shell
        for s in (0, 2):
            rec, mag = _sums_ref(x[0, b], x[1, b], *((None, None) if y is None else y), W, members[s])
            n = len(members[s])
            assert (np.abs(got[b, s] - rec) <= (n + 8) * 2.0 ** -52 * mag).all(), (b, s, got[b, s] - rec)
        if not with_target:
            assert (got[b, :, _hip.SP_SUM_YY:] == 0).all()
        single = _shell_sums(dev(x[:, b:b + 1]), None if y is None else dev(y), (D, H, W), index)
        assert np.array_equal(single[0], got[b])                          # row b does not depend on B
    again = _shell_sums(dev(x), None if y is None else dev(y), (D, H, W), index, fill=3.5, ws_fill=float("nan"))
    assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------ the driver
def _driver(est, target, plan, fill=SENTINEL, pivots=True):
    """ddpm3d_shell_spectrum through the C entry over sentinel-filled buffers -> (B, S, REC) numpy"""
    lib = _hip.load()
    est = est if est.dim() == 4 else est[None]
    B = est.shape[0]
    D, H, W = plan.shape
    axes, index, _ = plan.on(est.device)
    need = lib.ddpm3d_shell_spectrum_workspace_bytes(B, D, H, W, index.desc, int(target is not None))
    assert need >= 16 and need % 16 == 0
    ws = torch.full((need // 8,), fill, dtype=torch.float64, device="cuda")
    out = torch.full((B, plan.shells, _hip.SP_REC), fill, dtype=torch.float64, device="cuda")
    pe = plan.pivot(est) if pivots else None
    pt = plan.pivot(target[None]) if pivots and target is not None else None
    _hip.check(lib.ddpm3d_shell_spectrum(_hip.ptr(est), _hip.ptr(pe), _hip.ptr(target), _hip.ptr(pt), B, D, H, W,
                                         axes, index.desc, _hip.ptr(ws), need, _hip.ptr(out), _hip.stream()))
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def case():
    shape = (9, 33, 34)
    plan = metrics.spectrum_plan(shape, SPACING)
    v = _volumes(shape, 3, 4.0, seed=3)
    target = _volumes(shape, 1, 4.0, seed=5)[0]
    return shape, plan, v, target, _driver(dev(v), dev(target), plan)


def test_the_plan_index_is_the_restatement(case):
    shape, plan, v, target, rec = case
    axes, index, wins = plan.on(torch.device("cuda"))
    half = R.shell_numbers(shape, SPACING, half=True).reshape(-1)
    assert len(index) == plan.shells and index.counts == np.bincount(half, minlength=plan.shells).tolist()
    assert np.array_equal(index.index.cpu().numpy(), np.argsort(half, kind="stable"))
    assert plan.on(torch.device("cuda"))[1] is index                      # built once
    full = np.bincount(R.shell_numbers(shape, SPACING).reshape(-1), minlength=plan.shells)
    assert all(rec[b, :, _hip.SP_N].tolist() == full.tolist() for b in range(3))
    p = plan.pivot(dev(v)).cpu().numpy()
    assert p.dtype == np.float32 and p == pytest.approx([R.pivot(x, "hann") for x in v], rel=1e-6)


def test_driver_records_are_those_of_its_two_parts(case):
    shape, plan, v, target, rec = case
    x, y = dev(v), dev(target)
    xr, xi = metrics.dft3(x, plan, plan.pivot(x))
    yr, yi = metrics.dft3(y, plan, plan.pivot(y[None]))
    index = plan.on(x.device)[1]
    parts = _shell_sums((xr.reshape(3, -1), xi.reshape(3, -1)), (yr.reshape(-1), yi.reshape(-1)), shape, index)
    assert np.array_equal(parts, rec)
    assert np.array_equal(metrics.shell_spectrum(x, plan, y), rec)
    assert np.array_equal(metrics.shell_spectrum(x[1], plan, y)[0], rec[1])
    # against the restatement: a shell sum is within sum weight (2 |X| delta + delta^2) of its fp64 value
    want = R.shell_records(v, target, SPACING, "hann")
    sh = R.shell_numbers(shape, SPACING)
    Y = R.transform(target, "hann", np.float32(R.pivot(target, "hann")))
    dy = _bound(shape, _weighted(target[None], "hann", [np.float32(R.pivot(target, "hann"))]))
    for b in range(3):
        pb = np.float32(R.pivot(v[b], "hann"))
        X = R.transform(v[b], "hann", pb)
        dx = _bound(shape, _weighted(v[b:b + 1], "hann", [pb]))
        for s in range(plan.shells):
            ax, ay = np.abs(X[sh == s]), np.abs(Y[sh == s])
            ae = np.abs((X - Y)[sh == s])
            tol = {_hip.SP_SUM_XX: (2 * ax * dx + dx * dx).sum(), _hip.SP_SUM_YY: (2 * ay * dy + dy * dy).sum(),
                   _hip.SP_SUM_XY: (ax * dy + ay * dx + dx * dy).sum(),
                   _hip.SP_SUM_EE: (2 * ae * (dx + dy) + (dx + dy) ** 2).sum()}
            assert rec[b, s, _hip.SP_N] == want[b, s, R.N]
            for col, t in tol.items():
                assert abs(rec[b, s, col] - want[b, s, col]) <= t * (1 + 1e-9), (b, s, col)


def test_parseval(case):
    shape, plan, v, target, rec = case
    V = float(np.prod(shape))
    for b in range(3):
        pb = np.float32(R.pivot(v[b], "hann"))
        wv = _weighted(v[b:b + 1], "hann", [pb])[0]
        X = np.fft.fftn(wv)
        d = _bound(shape, wv)
        tol = (2 * np.abs(X) * d + d * d).sum()
        assert abs(rec[b, :, _hip.SP_SUM_XX].sum() - V * (wv ** 2).sum()) <= tol * (1 + 1e-9)


def test_estimate_is_target(case):
    shape, plan, v, target, rec = case
    x = dev(v[0])
    same = _driver(x, x, plan)[0]
    assert np.array_equal(same[:, _hip.SP_SUM_XY], same[:, _hip.SP_SUM_XX])
    assert np.array_equal(same[:, _hip.SP_SUM_YY], same[:, _hip.SP_SUM_XX])
    assert (same[:, _hip.SP_SUM_EE] == 0).all() and (same[:, _hip.SP_SUM_XX] > 0).all()
    assert np.array_equal(same[:, _hip.SP_SUM_XX], rec[0, :, _hip.SP_SUM_XX])
    fig = metrics.spectrum_figures(same, plan)
    assert fig["fsc"] == [1.0] * plan.n_reported and fig["ratio"] == [1.0] * plan.n_reported


def test_rows_do_not_depend_on_the_batch_and_a_nan_stays_in_its_row(case):
    shape, plan, v, target, rec = case
    y = dev(target)
    for b in range(3):
        assert np.array_equal(_driver(dev(v[b]), y, plan)[0], rec[b])
    bad = v.copy()
    bad[1, 4, 17, 20] = np.nan
    got = _driver(dev(bad), y, plan, pivots=False)
    clean = _driver(dev(v), y, plan, pivots=False)
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    for col in (_hip.SP_SUM_XX, _hip.SP_SUM_XY, _hip.SP_SUM_EE):
        assert not np.isfinite(got[1, :, col]).any()
    assert np.array_equal(got[1, :, _hip.SP_N], clean[1, :, _hip.SP_N])
    assert np.array_equal(got[1, :, _hip.SP_SUM_YY], clean[1, :, _hip.SP_SUM_YY])
    assert metrics.spectrum_figures(got, plan)[1]["fsc"] == [None] * plan.n_reported


def test_two_runs_give_the_same_bits_and_no_target_gives_zero_columns(case):
    shape, plan, v, target, rec = case
    assert np.array_equal(_driver(dev(v), dev(target), plan, fill=float("nan")), rec)
    alone = _driver(dev(v), None, plan)
    assert np.array_equal(alone, _driver(dev(v), None, plan, fill=1.0))
    assert (alone[:, :, _hip.SP_SUM_YY:] == 0).all()
    assert np.array_equal(alone[:, :, :_hip.SP_SUM_YY], rec[:, :, :_hip.SP_SUM_YY])


# ------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_outputs_alone(case):
    shape, plan, v, target, rec = case
    lib = _hip.load()
    D, H, W = shape
    Wh = W // 2 + 1
    x, y = dev(v), dev(target)
    axes, index, _ = plan.on(x.device)
    S = plan.shells
    big = 1 << 22
    ws = torch.full((big // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    re = torch.full((3, D, H, Wh), SENTINEL, dtype=torch.float32, device="cuda")
    im = torch.full((3, D, H, Wh), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((3, S, _hip.SP_REC), SENTINEL, dtype=torch.float64, device="cuda")
    P, st = _hip.ptr, _hip.stream()
    assert lib.ddpm3d_dft3_workspace_bytes(3, D, H, W) == (2 * 3 * D * H * Wh * 4 + 15) // 16 * 16 <= big
    assert lib.ddpm3d_shell_spectrum_workspace_bytes(3, D, H, W, index.desc, 1) <= big

    def axes_with(a, **kw):
        bad = (_hip.DftAxis * 3)(*[_hip.DftAxis(t.n, t.rows, t.cos_t, t.sin_t) for t in axes])
        for k, val in kw.items():
            setattr(bad[a], k, val)
        return bad

    def desc_with(**kw):
        d = index.desc
        bad = _hip.RoiIndex(d.regions, d.entries, d.offsets, d.d_offsets, d.d_chunks, d.d_index)
        for k, val in kw.items():
            setattr(bad, k, val)
        return bad

    def offsets_with(at, val):
        off = list(index.offsets)
        off[at] = val
        return (ctypes.c_int64 * len(off))(*off)

    def dft(vol=P(x), B=3, d=D, h=H, w=W, ax=axes, w_=P(ws), nbytes=big, r=P(re), i=P(im)):
        return lib.ddpm3d_dft3(vol, None, B, d, h, w, ax, w_, nbytes, r, i, st)

    def sums(xr=P(re), xi=P(im), yr=None, yi=None, B=3, d=D, h=H, w=W, ix=index.desc, w_=P(ws), nbytes=big, o=P(out)):
        return lib.ddpm3d_shell_sums(xr, xi, yr, yi, B, d, h, w, ix, w_, nbytes, o, st)

    def drv(e=P(x), t=P(y), B=3, d=D, h=H, w=W, ax=axes, ix=index.desc, w_=P(ws), nbytes=big, o=P(out)):
        return lib.ddpm3d_shell_spectrum(e, None, t, None, B, d, h, w, ax, ix, w_, nbytes, o, st)

    need_dft = lib.ddpm3d_dft3_workspace_bytes(3, D, H, W)
    need_sum = lib.ddpm3d_shell_sums_workspace_bytes(3, index.desc)
    need_drv = lib.ddpm3d_shell_spectrum_workspace_bytes(3, D, H, W, index.desc, 1)
    need_alone = lib.ddpm3d_shell_spectrum_workspace_bytes(3, D, H, W, index.desc, 0)
    assert need_alone < need_drv
    bad_index = [desc_with(regions=0), desc_with(regions=_hip.ROI_MAX_REGIONS + 1), desc_with(entries=-1),
                 desc_with(offsets=None), desc_with(d_offsets=None), desc_with(d_chunks=None), desc_with(d_index=None),
                 desc_with(offsets=offsets_with(0, 1)), desc_with(offsets=offsets_with(2, index.offsets[1] - 1)),
                 desc_with(offsets=offsets_with(S, index.offsets[S] - 1))]
    calls = [
        dft(vol=None), dft(r=None), dft(i=None), dft(w_=None), dft(ax=None), dft(B=0), dft(B=_hip.MAX_DRAWS + 1),
        dft(d=1), dft(h=1), dft(w=1), dft(d=_hip.SPEC_MAX_EXTENT + 1), dft(w=_hip.SPEC_MAX_EXTENT + 1),
        dft(ax=axes_with(0, n=D + 1)), dft(ax=axes_with(1, rows=H + 1)), dft(ax=axes_with(2, rows=W)),
        dft(ax=axes_with(2, n=W - 1)), dft(ax=axes_with(0, cos_t=None)), dft(ax=axes_with(2, sin_t=None)),
        dft(nbytes=need_dft - 1), dft(w_=P(ws) + 4),
        sums(xr=None), sums(xi=None), sums(o=None), sums(w_=None), sums(yr=P(re)), sums(yi=P(im)), sums(B=0),
        sums(B=_hip.MAX_DRAWS + 1), sums(d=1), sums(w=_hip.SPEC_MAX_EXTENT + 1), sums(ix=None),
        sums(nbytes=need_sum - 1), sums(w_=P(ws) + 8),
        drv(e=None), drv(o=None), drv(w_=None), drv(ax=None), drv(ix=None), drv(B=0), drv(B=_hip.MAX_DRAWS + 1),
        drv(h=1), drv(d=_hip.SPEC_MAX_EXTENT + 1), drv(ax=axes_with(1, n=H - 1)), drv(ax=axes_with(2, cos_t=None)),
        drv(w=W + 2),                                                    # entries no longer D H Wh (and the axes)
        drv(ix=desc_with(entries=index.desc.entries - 1)),
        drv(nbytes=need_drv - 1), drv(nbytes=need_alone),                # a target without room for it
        drv(w_=P(ws) + 8),
    ] + [sums(ix=d) for d in bad_index] + [drv(ix=d) for d in bad_index]
    assert calls == [_hip.E_INVAL] * len(calls), calls
    # nothing was launched: every buffer a launch of any of the three entries would write is still at the sentinel
    torch.cuda.synchronize()
    for name, buf in (("out", out), ("ws", ws), ("re", re), ("im", im)):
        assert bool((buf == SENTINEL).all()), name
    assert drv(t=None, nbytes=need_alone) == 0                           # ... which is room enough without one
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == SENTINEL).any())   # and that call did write
    # the queries: 0 for what the entries refuse, never smaller for a larger extent
    q = lib.ddpm3d_dft3_workspace_bytes
    assert [q(0, D, H, W), q(65, D, H, W), q(1, 1, H, W), q(1, D, H, 2049)] == [0] * 4
    assert q(1, D, H, W) <= q(1, D + 1, H, W) and q(1, D, H, W) <= q(1, D, H + 1, W) <= q(1, D, H + 1, W + 1)
    assert q(1, D, H, W) < q(2, D, H, W)
    assert lib.ddpm3d_shell_sums_workspace_bytes(0, index.desc) == 0
    assert lib.ddpm3d_shell_sums_workspace_bytes(1, bad_index[0]) == 0
    assert lib.ddpm3d_shell_spectrum_workspace_bytes(1, D, H, W + 2, index.desc, 1) == 0
    assert lib.ddpm3d_shell_spectrum_workspace_bytes(1, D, H, W, None, 1) == 0


# ------------------------------------------------------------------------------------------ the Python calls
def test_one_device_to_host_copy_per_call(case):
    """under torch's sync debug mode every blocking call warns: shell_spectrum makes one, the copy of its records"""
    shape, plan, v, target, rec = case
    x, y = dev(v), dev(target)
    metrics.shell_spectrum(x, plan, y)                                    # the library is loaded, the plan uploaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got = metrics.shell_spectrum(x, plan, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    blocking = [w for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(blocking) == 1, [str(w.message) for w in seen]
    assert np.array_equal(got, rec)


def test_the_three_single_passes_are_the_transform(case):
    """ddpm3d_dft3_pass (the timing entry) 0, 1, 2 in turn leave ddpm3d_dft3's bits; another pass number is refused"""
    shape, plan, v, target, rec = case
    lib = _hip.load()
    D, H, W = shape
    x = dev(v)
    pivot = plan.pivot(x)
    want = metrics.dft3(x, plan, pivot)
    axes = plan.on(x.device)[0]
    need = lib.ddpm3d_dft3_workspace_bytes(3, D, H, W)
    ws = torch.full((need // 4,), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((2, 3, D, H, W // 2 + 1), SENTINEL, dtype=torch.float32, device="cuda")
    call = lambda which: lib.ddpm3d_dft3_pass(which, _hip.ptr(x), _hip.ptr(pivot), 3, D, H, W, axes, _hip.ptr(ws),
                                              need, _hip.ptr(out[0]), _hip.ptr(out[1]), _hip.stream())
    assert call(3) == _hip.E_INVAL and call(-1) == _hip.E_INVAL
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (ws == SENTINEL).all()
    assert [call(0), call(1), call(2)] == [0, 0, 0]
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


def test_phantom_rows_on_the_device():
    """the README's phantom through the kernels: a stack gives the rows of its volumes, and the Gaussian shows in the
    ratio"""
    clean, low, smooth = R.phantom_rows()
    plan = metrics.spectrum_plan(clean.shape, (2.0, 2.0, 2.0))
    y = dev(clean)
    rows = metrics.spectrum_figures(metrics.shell_spectrum(dev(np.stack([low, smooth])), plan, y), plan)
    assert rows[0] == metrics.spectrum_figures(metrics.shell_spectrum(dev(low), plan, y), plan)[0]
    assert rows[1]["ratio"][-1] < 0.05 * rows[0]["ratio"][-1]             # the Gaussian takes the noise's power away
    assert rows[1]["ratio_half_mm"] is not None and rows[0]["ratio_half_mm"] is None


# ------------------------------------------------------------------------------------------ the script
FLAGS = ("--large_size 16 --small_size 16 --num_channels 32 --num_res_blocks 1 --num_head_channels 64 "
         "--attention_resolutions 1000 --learn_sigma True --resblock_updown True --use_scale_shift_norm True "
         "--timestep_respacing 3").split()
MM = (3.27, 2.0, 1.5)                                                      # along the file's (D, H, W)
SUMMARY = {"fsc_resolution_mm", "ratio_half_mm"}


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
    d = tmp_path_factory.mktemp("fsc")
    target = metrics_ref.phantom((24, 40, 40), seed=4)
    low = metrics_ref.noisy(target, 0.1, seed=4)
    np.savez(d / "pet.npz", low)
    np.savez(d / "full.npz", target)
    return d, target, low


def _strip(rep):
    rep = {k: v for k, v in rep.items() if k != "spectrum"}
    for name in ("denoised", "input"):
        rep[name] = {k: v for k, v in rep[name].items() if k != "spectrum"}
    if "baselines" in rep:
        rep["baselines"] = {n: {k: v for k, v in r.items() if k != "spectrum"} for n, r in rep["baselines"].items()}
    return rep


@pytest.mark.parametrize("path", ["one-shot", "joint", "draws", "draws-regions"])
def test_script_writes_the_spectrum_of_every_row(files, path):
    import json
    d, target, low = files
    mod = _script()
    extra = {"one-shot": ["--baseline_gaussian_fwhm", "5"], "joint": ["--joint_patches", "True"],
             "draws": ["--num_draws", "2"],                               # the draws pass through, one at a time
             "draws-regions": ["--num_draws", "2", "--roi_threshold_frac", "0.4"]}[path]   # held for the region block
    common = FLAGS + ["--base_samples", str(d / "pet.npz"), "--target_samples", str(d / "full.npz"),
                      "--voxel_spacing"] + [repr(s) for s in MM] + extra
    mod.main(common + ["--save_dir", str(d / path), "--spectrum", "True"])
    text = open(d / path / "metrics_pet.json").read()
    rep = json.loads(text)
    shape = (40, 40, 24)                                                   # (H, W, Z), as scored
    box = [[0, n] for n in shape] if path == "joint" else [[1, n - 1] for n in shape]
    cut = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0)[tuple(slice(a_, b_) for a_, b_ in box)])
    plan = metrics.spectrum_plan([b - a for a, b in box], (MM[1], MM[2], MM[0]))
    assert rep["spectrum"] == {"window": "hann", "shell_width": plan.shell_width, "shells": plan.shells,
                               "n_reported": plan.n_reported, "box": box}
    keys = {"frequency", "n", "power", "power_target", "power_error", "fsc", "ratio", "error_rel"} | SUMMARY
    rows = [rep["input"], rep["denoised"]] + list(rep.get("baselines", {}).values())
    assert len(rows) == (3 if path == "one-shot" else 2)
    for r in rows:
        assert set(r["spectrum"]) - {"draws"} == keys and len(r["spectrum"]["fsc"]) == plan.n_reported
        assert list(r)[-1] == "spectrum"                                   # added after everything the row had
    want = metrics.spectrum_figures(metrics.shell_spectrum(dev(cut(low)), plan, dev(cut(target))), plan)[0]
    assert rep["input"]["spectrum"] == json.loads(json.dumps(want))
    with_draws = path.startswith("draws")
    assert ("draws" in rep["denoised"]["spectrum"]) == with_draws and "draws" not in rep["input"]["spectrum"]
    if path == "draws-regions":                                            # the region block still got its K draws
        assert rep["roi"]["regions"] and all(len(r["denoised"]["draw_means"]) == 2 for r in rep["roi"]["regions"].values())
    if with_draws:
        each = rep["denoised"]["spectrum"]["draws"]
        assert len(each) == 2 and all(set(e) == SUMMARY for e in each) and each[0] != each[1]
    if path == "one-shot":
        assert rep["baselines"]["gaussian"]["spectrum"]["ratio"][-1] < rep["input"]["spectrum"]["ratio"][-1]
    log = open(d / path / "log.txt").read()
    assert log.count(" spectrum: FSC 0.5 at ") == len(rows)
    if path == "one-shot":
        # the same run without the flag: the file without the spectrum's keys, byte for byte, and no such log line
        mod.main(common + ["--save_dir", str(d / "plain")])
        plain = open(d / "plain" / "metrics_pet.json").read()
        assert '"spectrum"' not in plain and plain == json.dumps(_strip(rep), indent=2)
        assert " spectrum: " not in open(d / "plain" / "log.txt").read()
