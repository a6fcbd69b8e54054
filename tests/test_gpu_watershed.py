"""
GPU tier of the watershed split: ddpm3d_basins and ddpm3d_basin_saddles against the yardstick
(tests/watershed_ref.py).  Every output is an integer or a copied fp32 value, so the criterion is equality: peaks and
the reduced (pairs, saddle) with torch.equal, for connectivity 6, 18 and 26, on shapes that straddle one and two
workgroups of 256 voxels and a wave along every axis; random multi-label volumes with NaN and both infinities and
with heights of four levels only; a ramp, a serpentine path whose chain crosses every workgroup, constant plateaus;
the integer heights of a distance transform; split_components against the yardstick's split; the record capacity with
guard words behind the buffers; a short or missing workspace refused with every buffer untouched; the labelling and
the basins on one forest (ranked labels under a constant height); and the same bits on a second run.
"""

import functools

import numpy as np
import pytest
import torch

import edt_ref
import watershed_ref as R
from guided_diffusion import _hip, metrics

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (1, 1, 2), (3, 5, 7), (8, 8, 64), (9, 9, 65), (17, 10, 129))
CONNECTIVITIES = (6, 18, 26)
INF = float("inf")
GUARD = 64


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def case_of(shape, quantise):
    h, lab = R.random_case(shape, seed=sum(shape) + 7 * quantise, quantise=bool(quantise))
    h.setflags(write=False)
    lab.setflags(write=False)
    return h, lab


@functools.lru_cache(maxsize=None)
def want_of(shape, quantise, c):
    h, lab = case_of(shape, quantise)
    peaks, n, _ = R.basins(h, lab, c)
    return peaks, n, R.saddles(h, lab, peaks, c)


def raw_basins(h, lab, c, fill=None):
    """the C entry itself -> (peaks, status) tensors"""
    lib = _hip.load()
    D, H, W = h.shape
    peaks = torch.empty(h.shape, dtype=torch.int32, device="cuda")
    if fill is not None:
        peaks.fill_(fill)
    ws = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    _hip.check(lib.ddpm3d_basins(_hip.ptr(h), _hip.ptr(lab), c, D, H, W, _hip.ptr(peaks), _hip.ptr(ws), 16,
                                 _hip.ptr(status), _hip.stream()))
    return peaks, status


def raw_saddles(h, lab, peaks, c, cap):
    """the C entry itself with GUARD words of a pattern behind both record buffers -> (pairs, saddle, status, intact)"""
    lib = _hip.load()
    D, H, W = h.shape
    pairs = torch.full((2 * cap + GUARD,), -12345, dtype=torch.int32, device="cuda")
    saddle = torch.full((cap + GUARD,), -777.0, dtype=torch.float32, device="cuda")
    ws = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    _hip.check(lib.ddpm3d_basin_saddles(_hip.ptr(h), _hip.ptr(lab), _hip.ptr(peaks), c, D, H, W, cap,
                                        _hip.ptr(pairs), _hip.ptr(saddle), _hip.ptr(ws), 16, _hip.ptr(status),
                                        _hip.stream()))
    intact = bool((pairs[2 * cap:] == -12345).all()) and bool((saddle[cap:] == -777.0).all())
    return pairs[:2 * cap].reshape(cap, 2), saddle[:cap], status.cpu().tolist(), intact


def check_against_yardstick(h, lab, c, want=None):
    """basins and basin_saddles on host arrays h, lab against the yardstick -> (n_basins, n_edges)"""
    if want is None:
        want_peaks, n, _ = R.basins(h, lab, c)
        want = (want_peaks, n, R.saddles(h, lab, want_peaks, c))
    want_peaks, n, (want_pairs, want_saddle) = want
    dh, dl = dev(h), dev(lab)
    peaks, got_n = metrics.basins(dh, dl, c)
    assert got_n == n
    assert torch.equal(peaks.cpu(), torch.from_numpy(np.ascontiguousarray(want_peaks)))
    pairs, saddle = metrics.basin_saddles(dh, dl, peaks, c)
    assert pairs.dtype == torch.int32 and saddle.dtype == torch.float32
    assert torch.equal(pairs.cpu(), torch.from_numpy(want_pairs))
    assert torch.equal(saddle.cpu(), torch.from_numpy(want_saddle))
    return n, int(want_pairs.shape[0])


# ------------------------------------------------------------------------------------------ the two entries
@pytest.mark.parametrize("c", CONNECTIVITIES)
@pytest.mark.parametrize("quantise", [0, 1], ids=["random", "four-levels"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_basins_and_saddles_equal_the_yardstick(shape, quantise, c):
    h, lab = case_of(shape, quantise)
    n, edges = check_against_yardstick(h, lab, c, want_of(shape, quantise, c))
    if np.prod(shape) > 1000:
        assert n > 10 and edges > 10                     # the case does exercise the saddle graph
        assert np.isnan(h).any() and np.isinf(h).any()


def test_labels_that_touch_do_not_connect():
    """two labels side by side under a rising ramp: with one label the ramp is one basin, with two each has its own
    peak and no saddle joins them"""
    h = np.arange(3 * 4 * 40, dtype=np.float32).reshape(3, 4, 40)
    lab = np.ones(h.shape, dtype=np.int32)
    assert check_against_yardstick(h, lab, 26) == (1, 0)
    lab[:, :, 17:] = 2
    assert check_against_yardstick(h, lab, 26) == (2, 0)
    lab[:, 2:, :] += 2
    assert check_against_yardstick(h, lab, 6) == (4, 0)


@pytest.mark.parametrize("rising", [True, False], ids=["rising", "falling"])
def test_ramp_of_300(rising):
    h, lab = R.ramp(300, rising)
    _, n, longest = R.basins(h, lab, 6)
    assert (n, longest) == (1, 299)
    for c in CONNECTIVITIES:
        assert check_against_yardstick(h, lab, c) == (1, 0)


def test_serpentine_is_one_basin():
    h, lab, length = R.serpentine((9, 9, 70))
    want = R.basins(h, lab, 6)
    assert length > 1500 and want[1] == 1 and want[2] == length - 1      # the chain is the whole path
    peaks, status = raw_basins(dev(h), dev(lab), 6)
    assert status.cpu().tolist() == [0, 1]                               # cap flag 0, one peak
    assert torch.equal(peaks.cpu(), torch.from_numpy(want[0]))
    assert check_against_yardstick(h, lab, 6, (want[0], 1, R.saddles(h, lab, want[0], 6))) == (1, 0)


def test_constant_plateaus():
    h, lab = R.constant_box((9, 17, 130))
    peaks, n = metrics.basins(dev(h), dev(lab), 26)
    assert n == 1 and int(peaks.min()) == 0 and int(peaks.max()) == 0    # one basin, at voxel 0
    for c in CONNECTIVITIES:
        assert check_against_yardstick(h, lab, c) == (1, 0)
    h, lab = R.u_plateau()
    for c in CONNECTIVITIES:
        n, _ = check_against_yardstick(h, lab, c)
        assert n > 1
        out, pieces, info = metrics.split_components(dev(lab), dev(h), 1e-9, connectivity=c)
        assert pieces == 1 and info["n_basins"] == n and torch.equal(out.cpu(), torch.from_numpy(lab))


def test_distance_transform_heights_split_two_balls():
    """the classical split of touching blobs by shape: integer heights, the tie-break's hardest case"""
    mask = R.two_balls()
    lab, n = metrics.label_components(dev(mask.astype(np.float32)), 0.5)
    assert n == 1
    h = metrics.distance_sq(dev(mask), (1.0, 1.0, 1.0))
    want_h = edt_ref.distance_sq(mask, (1.0, 1.0, 1.0)).astype(np.float32)
    assert torch.equal(h.cpu(), torch.from_numpy(want_h))                # exact at unit spacing
    hh, ll = h.cpu().numpy(), lab.cpu().numpy()
    assert np.array_equal(hh, np.round(hh))
    for c in CONNECTIVITIES:
        check_against_yardstick(hh, ll, c)
    want, n_want, info_want = R.split(ll, hh, 2.0, 26)
    got, n_got, info = metrics.split_components(lab, h, 2.0)
    assert n_want == 2 and n_got == 2 and info == info_want
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ------------------------------------------------------------------------------------------ split_components
@pytest.mark.parametrize("c", [6, 26])
@pytest.mark.parametrize("noise", [0.0, 0.1], ids=["clean", "noisy"])
def test_split_components_on_the_two_blobs(noise, c):
    h, lab = R.two_blobs(noise=noise)
    dh, dl = dev(h), dev(lab)
    counts = []
    for P in (0.0, 0.05, 0.1, 0.2, 0.3, 0.5, INF):
        want, n_want, info_want = R.split(lab, h, P, c)
        got, n, info = metrics.split_components(dl, dh, P, connectivity=c)
        assert got.dtype == torch.int32 and got.is_cuda and n == n_want and info == info_want, (P, info, info_want)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), P
        assert info["n_after"] == n and len(info["parent"]) == n and set(info["parent"]) == {1}
        counts.append(n)
    assert counts[0] == info["n_basins"] and counts[-1] == 1 and counts == sorted(counts, reverse=True)
    if noise == 0.0:
        assert counts[:3] == [2, 2, 2] and np.bincount(
            metrics.split_components(dl, dh, 0.05, connectivity=c)[0].cpu().numpy().reshape(-1))[1:].tolist() == [779, 545]


def test_split_components_parents_and_infinite_prominence():
    """P = inf gives back segment's labels on the phantom; a finite P names each piece's component"""
    clean, low, _ = edt_ref.phantom_rows()
    vol = dev(clean)
    lab, n = metrics.segment(vol, 0.5 * float(clean.max()), min_voxels=2)
    assert n >= 2
    got, n_got, info = metrics.split_components(lab, vol, INF)
    assert n_got == n and torch.equal(got, lab) and info["parent"] == list(range(1, n + 1))
    assert info["n_before"] == n and info["n_after"] == n
    noisy = dev(low)
    got, n_got, info = metrics.split_components(lab, noisy, 0.02)
    want, n_want, info_want = R.split(lab.cpu().numpy(), low, 0.02)
    assert n_got == n_want > n and info == info_want and torch.equal(got.cpu(), torch.from_numpy(want))
    g, l = got.cpu().numpy(), lab.cpu().numpy()
    assert np.array_equal(g > 0, l > 0)
    for piece, old in enumerate(info["parent"], start=1):
        assert (l[g == piece] == old).all()                                  # a piece lies in one component: its parent
    assert sorted(set(info["parent"])) == list(range(1, n + 1))
    with pytest.raises(ValueError, match="smooth"):
        metrics.split_components(lab, noisy, 0.02, max_basins=info["n_basins"] - 1)


# ------------------------------------------------------------------------------------------ capacity, repeatability
@pytest.mark.parametrize("c", CONNECTIVITIES)
def test_record_capacity(c):
    shape = (9, 9, 65)
    h, lab = case_of(shape, 0)
    want_peaks, _, (want_pairs, want_saddle) = want_of(shape, 0, c)
    dh, dl, peaks = dev(h), dev(lab), dev(want_peaks)
    _, _, (flag, need), intact = raw_saddles(dh, dl, peaks, c, 0)            # cap = 0 is legal: it sizes the next call
    assert flag == 0 and need >= len(want_pairs) > 0 and intact
    small = need // 2
    pairs, saddle, (flag, need2), intact = raw_saddles(dh, dl, peaks, c, small)
    assert flag == 0 and need2 == need and intact                            # counted, never written
    assert bool((pairs[:, 0] < pairs[:, 1]).all()) and bool((pairs >= 0).all())
    pairs, saddle, (flag, need3), intact = raw_saddles(dh, dl, peaks, c, need)
    assert flag == 0 and need3 == need and intact
    got_pairs, got_saddle = metrics.reduce_saddles(pairs, saddle)
    assert torch.equal(got_pairs.cpu(), torch.from_numpy(want_pairs))
    assert torch.equal(got_saddle.cpu(), torch.from_numpy(want_saddle))
    print("connectivity %d: %d records for %d edges, duplication %.2f" % (c, need, len(want_pairs),
                                                                         need / len(want_pairs)))
    # the Python entry makes its second call when the first buffer is too small, and the same graph comes out
    calls = []
    inner = metrics._saddle_records

    def counted(*a):
        calls.append(a[-1])
        return inner(*a)

    metrics._saddle_records = counted
    try:
        again = metrics.basin_saddles(dh, dl, peaks, c, capacity=small)
    finally:
        metrics._saddle_records = inner
    assert calls == [small, need]
    assert torch.equal(again[0], got_pairs) and torch.equal(again[1], got_saddle)


@pytest.mark.parametrize("entry", ["basins", "basin_saddles"])
def test_a_short_or_missing_workspace_is_refused(entry):
    lib = _hip.load()
    shape = (9, 9, 65)
    h, lab = case_of(shape, 0)
    dh, dl = dev(h), dev(lab)
    need = getattr(lib, "ddpm3d_%s_workspace_bytes" % entry)(*shape)
    assert need > 0 and need % 16 == 0
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device="cuda")
    peaks = torch.full(shape, -77, dtype=torch.int32, device="cuda")
    pairs = torch.full((8, 2), -12345, dtype=torch.int32, device="cuda")
    saddle = torch.full((8,), -777.0, dtype=torch.float32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    for ws_ptr, ws_bytes in ((_hip.ptr(ws), need - 1), (None, need)):
        tail = (ws_ptr, ws_bytes, _hip.ptr(status), _hip.stream())
        if entry == "basins":
            rc = lib.ddpm3d_basins(_hip.ptr(dh), _hip.ptr(dl), 26, *shape, _hip.ptr(peaks), *tail)
        else:
            rc = lib.ddpm3d_basin_saddles(_hip.ptr(dh), _hip.ptr(dl), _hip.ptr(peaks), 26, *shape, 8, _hip.ptr(pairs),
                                          _hip.ptr(saddle), *tail)
        assert rc == _hip.E_INVAL, (rc, ws_bytes)
        assert lib.ddpm3d_last_error().decode().startswith("%s: needs %d bytes" % (entry, need))
        torch.cuda.synchronize()
        assert bool((peaks == -77).all()) and status.tolist() == [-7, -7] and bool((ws == 0x5a).all())
        assert bool((pairs == -12345).all()) and bool((saddle == -777.0).all())


@pytest.mark.parametrize("c", CONNECTIVITIES)
def test_labelling_and_basins_agree_on_one_forest(c):
    """ddpm3d_label_components' ranked labels under a constant height: what the two definitions give, no more"""
    import segment_ref
    lib = _hip.load()
    shape = (9, 9, 65)
    mask = segment_ref.random_mask(shape, 0.5, seed=90 + c)
    want_labels, n = segment_ref.label(mask, c)
    vol = dev(np.where(mask, 1.0, 0.0).astype(np.float32))
    need = lib.ddpm3d_label_components_workspace_bytes(*shape)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    roots = torch.empty(shape, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    _hip.check(lib.ddpm3d_label_components(_hip.ptr(vol), None, 0.5, c, *shape, _hip.ptr(roots), _hip.ptr(ws), need,
                                           _hip.ptr(status), _hip.stream()))
    assert status.tolist() == [0, n]
    assert np.array_equal(roots.cpu().numpy(), segment_ref.roots(want_labels))
    labels, got_n = metrics.label_components(vol, 0.5, connectivity=c)
    assert got_n == n and np.array_equal(labels.cpu().numpy(), want_labels)

    height = np.full(shape, 2.5, dtype=np.float32)
    want_peaks, n_peaks, _ = R.basins(height, want_labels, c)
    peaks, status = raw_basins(dev(height), labels, c)
    assert status.tolist() == [0, n_peaks] and n_peaks >= n
    peaks = peaks.cpu().numpy()
    assert np.array_equal(peaks, want_peaks)
    assert np.array_equal(peaks >= 0, mask)
    served = peaks[mask]                                                    # the peak of every foreground voxel
    flat_labels, flat_peaks = want_labels.reshape(-1), peaks.reshape(-1)
    assert np.array_equal(flat_labels[served], want_labels[mask]) and (flat_labels[served] > 0).all()
    assert np.array_equal(flat_peaks[served], served)


@pytest.mark.parametrize("c", CONNECTIVITIES)
def test_two_runs_give_the_same_bits(c):
    shape = (17, 10, 129)
    h, lab = case_of(shape, 1)
    dh, dl = dev(h), dev(lab)
    first, status1 = raw_basins(dh, dl, c, fill=0)
    second, status2 = raw_basins(dh, dl, c, fill=-1)                         # whatever the buffer held before
    assert torch.equal(first, second) and torch.equal(status1, status2) and int(status1[0]) == 0
    a = metrics.basin_saddles(dh, dl, first, c)
    b = metrics.basin_saddles(dh, dl, second, c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
