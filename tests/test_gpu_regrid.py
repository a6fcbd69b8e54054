"""
GPU tier of volume regridding: ddpm3d_regrid through regrid.apply, and once through the raw entry,
against the fp64 yardstick of tests/regrid_ref.py, every voxel within the composed bound of the fma chains; growing
and shrinking axes, identity axes skipped with one, two and three passes, the most taps the tables reach, rows that
cross wave and block edges, unit extents, data on an offset; a stack against its single calls, two runs, the input
left alone, no pass at all; where a NaN may show and where not; a table that lies about its counts; keep_after.

Largest share of the bound used in one run on an MI355X: 0.98 on a single linear pass with two taps, 0.73 to 0.83 on
the other single passes over short rows, 0.03 to 0.61 elsewhere; 0.39 and 0.31 on the offset data.
"""

import numpy as np
import pytest
import torch

import regrid_ref as R
from guided_diffusion import _hip, regrid

pytestmark = pytest.mark.gpu

# shape_in, shape_out, mode
CASES = {
    "grow": ((5, 6, 7), (9, 11, 20), "linear"),
    "grow_cubic": ((5, 6, 7), (9, 11, 20), "cubic"),
    "shrink": ((13, 17, 19), (5, 7, 6), "linear"),
    "shrink_cubic": ((13, 17, 19), (5, 7, 6), "cubic"),
    "mixed_two_passes": ((12, 9, 33), (12, 20, 11), "linear"),      # D is the identity: W and H run
    "one_pass_W": ((4, 9, 33), (4, 9, 11), "cubic"),
    "one_pass_H": ((4, 9, 33), (4, 20, 33), "linear"),
    "one_pass_D": ((12, 9, 33), (7, 9, 33), "cubic"),
    "two_passes_H_D": ((12, 9, 33), (7, 20, 33), "linear"),         # W is the identity: the H pass reads vol
    "two_passes_W_D": ((12, 9, 33), (30, 9, 70), "cubic"),
    "max_taps": ((2, 3, 68), (2, 3, 17), "cubic"),
    "Wo_63": ((3, 5, 40), (3, 5, 63), "linear"),
    "Wo_64": ((3, 5, 100), (3, 5, 64), "cubic"),
    "Wo_65": ((3, 5, 40), (3, 7, 65), "cubic"),
    "Wo_257": ((2, 3, 90), (3, 2, 257), "linear"),
    "unit_extents": ((1, 6, 1), (1, 11, 1), "cubic"),
    "unit_in_grows": ((1, 1, 5), (3, 4, 9), "linear"),
    "shrinks_to_unit": ((4, 3, 7), (1, 1, 2), "cubic"),
    # the H and D passes move 16 bytes per lane where the row length is a multiple of 4 and at least 128 words
    "row_124_below_the_threshold": ((3, 5, 124), (3, 7, 124), "linear"),
    "row_128_at_the_threshold": ((3, 5, 128), (3, 7, 128), "linear"),
    "row_130_no_multiple_of_4": ((3, 5, 130), (3, 7, 130), "cubic"),
    "row_132_part_of_a_wave": ((3, 5, 132), (5, 7, 132), "cubic"),         # 21 rows: no multiple of the 4 per workgroup
    "row_260_two_chunks_14_taps": ((9, 17, 260), (4, 5, 260), "cubic"),
    "row_8_taps": ((8, 16, 128), (4, 8, 128), "cubic"),
    "row_after_a_voxel_pass": ((6, 7, 40), (9, 11, 128), "linear"),        # W by voxels, H and D by rows
}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared references are read-only


def bits(t):
    return t.contiguous().view(torch.int32)


def within_bound(got, mean, bound, what):
    """every voxel within the bound of the yardstick; prints the largest share of the bound used"""
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == mean.shape
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - mean)
    used = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s: largest deviation %.3g = %.4g of the bound" % (what, float(err.max()), used))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float(err.max()), used)
    return used


@pytest.fixture(scope="module")
def references():
    out = {}
    for seed, (name, (shape_in, shape_out, mode)) in enumerate(sorted(CASES.items())):
        x = R.data(shape_in, 100 + seed) - np.float32(0.25)             # both signs
        x.setflags(write=False)
        out[name] = (x,) + R.apply(x, shape_out, mode)
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_voxel_within_the_composed_bound(case, references):
    shape_in, shape_out, mode = CASES[case]
    x, m, bound = references[case]
    plan = regrid.plan(shape_in, shape_out, mode)
    if case == "max_taps":
        assert plan.axes[2].taps == 16 == int(plan.axes[2].count.max())     # the most any ratio in [1/4, 4] gives
    vol = dev(x)
    got = regrid.apply(vol, plan)
    assert tuple(got.shape) == shape_out
    within_bound(got, m, bound, "%s %s -> %s %s" % (case, shape_in, shape_out, mode))
    assert torch.equal(bits(vol), bits(dev(x)))                              # vol is only read


@pytest.mark.parametrize("mode", ["linear", "cubic"])
def test_data_on_an_offset(mode):
    """a mean of 4 under a signal of 1: the bound scales with sum |w| |x|, and so must the error"""
    shape_in, shape_out = (9, 10, 21), (14, 6, 30)
    x = R.data(shape_in, 7, offset=4.0)
    m, bound = R.apply(x, shape_out, mode)
    within_bound(regrid.apply(dev(x), regrid.plan(shape_in, shape_out, mode)), m, bound, "offset 4 " + mode)


def test_a_stack_equals_its_single_calls_and_two_runs_agree():
    shape_in, shape_out = (7, 9, 33), (10, 5, 70)
    plan = regrid.plan(shape_in, shape_out, "cubic")
    x = dev(R.data((3,) + shape_in, 11, offset=-0.5))
    stack = regrid.apply(x, plan)
    assert tuple(stack.shape) == (3,) + shape_out
    for b in range(3):
        assert torch.equal(bits(stack[b]), bits(regrid.apply(x[b].contiguous(), plan)))
    assert torch.equal(bits(stack), bits(regrid.apply(x, plan)))
    m, bound = R.apply(x.cpu().numpy(), shape_out, "cubic")
    within_bound(stack, m, bound, "stack of 3")


def test_the_two_kernels_of_a_pass_give_the_same_bits():
    """the same volume 4 bytes off a 16-byte boundary cannot take the 16-byte loads: the H pass then runs voxel by
    voxel, and must give what the row kernel gives"""
    shape_in, shape_out = (3, 9, 256), (3, 14, 256)
    for mode in ("linear", "cubic"):
        plan = regrid.plan(shape_in, shape_out, mode)
        x = dev(R.data(shape_in, 21))
        buf = torch.zeros(x.numel() + 8, dtype=torch.float32, device="cuda")
        off = buf[1:1 + x.numel()].view(shape_in)
        off.copy_(x)
        assert x.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert torch.equal(bits(regrid.apply(x, plan)), bits(regrid.apply(off, plan)))


def test_no_pass_at_all_gives_a_copy():
    x = dev(R.data((2, 5, 6, 7), 12))
    plan = regrid.plan((5, 6, 7), (5, 6, 7), "cubic")
    assert plan.identity
    for vol in (x, x[0].contiguous()):
        got = regrid.apply(vol, plan)
        assert got.data_ptr() != vol.data_ptr() and torch.equal(bits(got), bits(vol))


@pytest.mark.parametrize("mode", ["linear", "cubic"])
@pytest.mark.parametrize("shapes", [((6, 7, 20), (9, 4, 13)), ((5, 6, 68), (5, 6, 17)), ((5, 6, 7), (5, 6, 7))], ids=str)
def test_a_nan_shows_exactly_where_the_tables_say(shapes, mode):
    """a kernel that reads a tap at or beyond count[o] (weight 0) would spread the NaN further: 0 * NaN is NaN"""
    shape_in, shape_out = shapes
    x = R.data(shape_in, 13)
    at = tuple(n // 2 for n in shape_in)
    x[at] = np.nan
    want = R.nonfinite_after(np.isnan(x), shape_out, mode)
    got = ~torch.isfinite(regrid.apply(dev(x), regrid.plan(shape_in, shape_out, mode))).cpu().numpy()
    assert 0 < want.sum() < want.size and np.array_equal(got, want)
    # and at a face, where the window is cut
    y = R.data(shape_in, 14)
    y[0, 0, 0] = y[-1, -1, -1] = np.inf
    want = R.nonfinite_after(np.isinf(y), shape_out, mode)
    got = ~torch.isfinite(regrid.apply(dev(y), regrid.plan(shape_in, shape_out, mode))).cpu().numpy()
    assert np.array_equal(got, want)


def _raw(vol, shape_out, tables, B=1):
    """ddpm3d_regrid itself on device tables given as (taps, first, count, weights [tap][out_len]) or None per axis"""
    lib = _hip.load()
    shape_in = tuple(vol.shape[-3:])
    axes, keep = (_hip.RegridAxis * 3)(), []
    for i, t in enumerate(tables):
        axes[i].in_len, axes[i].out_len, axes[i].taps = shape_in[i], shape_out[i], 0
        if t is not None:
            taps, first, count, weights = t
            held = [torch.tensor(first, dtype=torch.int32).cuda(), torch.tensor(count, dtype=torch.int32).cuda(),
                    torch.tensor(weights, dtype=torch.float32).cuda().contiguous()]
            assert tuple(held[2].shape) == (taps, shape_out[i])
            axes[i].taps = taps
            axes[i].first, axes[i].count, axes[i].weights = (h.data_ptr() for h in held)
            keep.append(held)
    need = lib.ddpm3d_regrid_workspace_bytes(B, *shape_in, *shape_out)
    assert need > 0
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full(((B,) if vol.dim() == 4 else ()) + tuple(shape_out), float("nan"), dtype=torch.float32,
                     device="cuda")
    rc = lib.ddpm3d_regrid(vol.data_ptr(), B, *shape_in, axes, out.data_ptr(), ws.data_ptr(), need,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def test_the_raw_entry_equals_apply():
    shape_in, shape_out = (6, 7, 20), (9, 7, 13)
    plan = regrid.plan(shape_in, shape_out, "cubic")
    x = dev(R.data((2,) + shape_in, 15))
    tables = [None if a.identity else (a.taps, a.first.tolist(), a.count.tolist(), a.weights.T.tolist())
              for a in plan.axes]
    rc, out = _raw(x, shape_out, tables, B=2)
    assert rc == 0 and torch.equal(bits(out), bits(regrid.apply(x, plan)))


def test_a_table_that_lies_gives_numbers_and_reads_nothing_outside_vol():
    """count above the tap capacity and first + count beyond the axis, first below 0 and beyond the axis: the kernel
    clamps count to 0..taps and every index to 0..Li - 1, so the entry succeeds and the output is finite.  The volume
    sits between two NaN walls of one allocation: an index that left it by less than a wall would show."""
    shape_in, shape_out, taps = (3, 4, 10), (3, 4, 6), 3
    wall = 3 * 4 * 10
    buf = torch.full((3 * wall,), float("nan"), dtype=torch.float32, device="cuda")
    buf[wall:2 * wall] = dev(R.data(shape_in, 16)).reshape(-1)
    vol = buf[wall:2 * wall].view(shape_in)
    first = [8, 9, 20, -5, 0, 2 ** 31 - 1]
    count = [7, 100, 3, 3, 2 ** 31 - 1, -4]
    weights = [[0.5] * 6, [0.25] * 6, [0.25] * 6]
    rc, out = _raw(vol, shape_out, [None, None, (taps, first, count, weights)])
    assert rc == 0
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    x = vol.cpu().numpy().astype(np.float64)
    # what the clamps make of it: count -> min(max(count, 0), taps), first -> into the axis, indices -> at most Li - 1
    for o, (f, n) in enumerate(zip(first, count)):
        n, f = min(max(n, 0), taps), min(max(f, 0), 9)
        want = sum(np.float64(np.float32(weights[t][o])) * x[:, :, min(f + t, 9)] for t in range(n))
        assert np.abs(got[:, :, o] - want).max() <= 1e-6, o
    assert (got[:, :, 5] == 0).all()                                    # no counted tap: the empty sum


@pytest.mark.parametrize("mode", ["linear", "cubic"])
def test_keep_after_on_zero_faces_and_an_interior_hole(mode):
    shape_in, shape_out = (10, 12, 14), (7, 12, 30)
    keep = np.ones(shape_in, dtype=np.uint8)
    keep[0] = keep[-1] = 0
    keep[:, 0] = keep[:, -1] = 0
    keep[:, :, 0] = keep[:, :, -1] = 0
    keep[5, 6, 7] = 0
    want = R.keep_after(keep, shape_out, mode)
    plan = regrid.plan(shape_in, shape_out, mode)
    got = regrid.keep_after(dev(keep), plan)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == shape_out
    assert 0 < want.sum() < want.size and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(regrid.keep_after(dev(np.ones(shape_in, np.uint8)), plan).cpu().numpy(),
                          np.ones(shape_out, np.uint8))
    for bad in (dev(keep).float(), dev(keep)[:, :, ::2], dev(keep)[1:]):
        with pytest.raises(ValueError, match="regrid.keep_after"):
            regrid.keep_after(bad, plan)


def test_apply_refusals_with_real_tensors():
    plan = regrid.plan((4, 5, 6), (8, 5, 3))
    x = torch.zeros((4, 5, 6), device="cuda")
    for bad, names in ((x.double(), "contiguous float32"), (x.permute(0, 2, 1), "contiguous float32"),
                       (x[:, :, :5], "contiguous float32"), (x[None, None], "the plan takes"),
                       (torch.zeros((4, 5, 7), device="cuda"), "the plan takes"),
                       (torch.zeros((65, 4, 5, 6), device="cuda"), "65 volumes")):
        with pytest.raises(ValueError, match=names):
            regrid.apply(bad, plan)
    assert tuple(regrid.apply(x, plan).shape) == (8, 5, 3)
    assert tuple(regrid.apply(torch.zeros((64, 4, 5, 6), device="cuda"), plan).shape) == (64, 8, 5, 3)
