"""
The streaming attention kernels (csrc/attention.hip: exact fp32 MFMA and f16x3, head widths 32 / 64 / 128) at the
places where such kernels fail, through ddpm3d_attention_p, against the fp64 reference of attention_ref.py:

  (a) bound conventions   the network's own wiring (a 1x1 qkv conv with statistics -> the bounds-only gn_finalize
                          -> (pointer + 1 float, 32 entries, stride 2)), hand-built interleaved entries with the
                          maximum in one entry, 1 / 33 / 64 entries, loose bounds, the mantissa extremes, the
                          degenerate bounds 0 and inf, an understated bound, per-sample magnitudes 2^27 apart
  (b) the recurrence      the running max rising in every tile, falling, rising for every other query of a wave,
                          sitting in the ragged last tile; all logits <= -10 beside zero-padded keys; identical
                          keys; one-hot weights whose alpha underflows to 0
  (c) edges               T = 1 .. 257 around the 32-key tile and the 128-query block with a head 2^-12 of the
                          other; guard rows around qkv and out
  (d) argument checks     everything ddpm3d_attention_p refuses, before any launch

The figure is max|got - ref| / max|ref| per (sample, head), bar 1e-5 (the bar of
test_attention_core_vs_legacy_reference), and max_c|err| / max_c|ref| per query row of a head, bar 1e-4 (the
long-sequence test's); both arithmetic modes meet the same bars.  Every launch is made twice and the outputs are
bitwise equal.  The cases, their guarantees (asserted in fp64 by their builders) and the mutations they are there
for: attention_ref.py and test_attention_model_cpu.py.

Measured on an MI355X, worst per (sample, head) figure per group: see DESIGN.md ("Attention at its edges").
"""

import numpy as np
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu

MODES = {0: "f32", 1: "f16x3"}
GUARD = 128             # guard rows on either side of qkv and out
SENTINEL = 0x7a5a5a5a   # bits of the float (2.8e35) that fills out and its guards before a launch


@pytest.fixture(scope="module")
def hc():
    import hipcall
    return hipcall


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _launch(c, precision, qkv_dev=None, bound_dev=None, null_bound=False):
    """one ddpm3d_attention_p call on case c: NaN-pre-filled output -> numpy"""
    import guided_diffusion._hip as H
    lib = H.load()
    qd = torch.tensor(c.qkv).cuda() if qkv_dev is None else qkv_dev
    bd = torch.tensor(c.bound).cuda() if bound_dev is None else bound_dev
    out = torch.full((c.N, c.T, c.heads * c.ch), float("nan"), device="cuda")
    args = (0, 0, 0) if null_bound else (bd.data_ptr() + 4 * c.offset, c.count, c.stride)
    H.check(lib.ddpm3d_attention_p(H.ptr(qd), c.N, c.T, c.heads, c.ch, precision, *args, H.ptr(out), H.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _run(c, precision, **dev):
    """two launches, bitwise equal.  The exact mode's second launch passes no bound at all (null, 0, 0): it must
    ignore the bound entirely."""
    got = _launch(c, precision, **dev)
    again = _launch(c, precision, null_bound=(precision == 0), **dev)
    assert np.array_equal(_bits(got), _bits(again))
    return got


def _hold_to_the_bars(c, got, ref, precision):
    assert np.isfinite(got).all()
    per_head, per_row = R.head_errors(got, ref, c.heads, c.ch)
    print("attention (%s) %s %s: per (sample, head) %.3g, per row %.3g"
          % (c.group, c.name, MODES[precision], per_head.max(), per_row.max()))
    assert per_head.max() < R.BAR, per_head
    assert per_row.max() < R.ROW_BAR


def _check(c, got, precision):
    ref = R.case_reference(c.name) if c.name in R.CASES else R.reference(c.qkv, c.heads, c.ch)
    if c.kind == "zero":
        assert (got == 0).all()
        return
    if c.kind == "onehot":
        sel, bound = R.one_hot_expected(c)
        if precision == 0:
            assert np.array_equal(got, sel.astype(np.float32))          # the matching v row, bit for bit
        else:
            worst = float((np.abs(got - sel) / bound).max())
            print("attention (b) %s f16x3: %.3g of the element bound" % (c.name, worst))
            assert worst <= 1.0
    _hold_to_the_bars(c, got, ref, precision)


# ---------------------------------------------------------------------------------------------------------------
# (a) bound conventions
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
def test_network_wiring_of_the_bound(hc, precision):
    """What the launch plan does (unet_plan.hip, engine.py: attention): the qkv 1x1 conv writes its statistics,
    the bounds-only ddpm3d_gn_finalize turns them into [N][32][2] upper bounds, and the attention kernel gets
    (that pointer + 4 bytes, 32, 2).  Each of the 32 entries read back bounds the true |qkv| of its group (asserted
    by wiring_case; they are upper bounds, up to 40x loose), sample 1 is a thousandth of sample 0, and the result
    is held to the bars against the reference on the conv's actual output."""
    import guided_diffusion._hip as H
    lib = H.load()
    heads, ch = 2, 32
    x, w, b = R.wiring_qkv_inputs(heads, ch)
    N, dhw = x.shape[0], x.shape[2:]
    T, co = int(np.prod(dhw)), heads * 3 * ch
    qkv, stats, _ = hc.conv3d([hc.to_ndhwc(torch.tensor(x)).cuda()], torch.tensor(w).cuda(), torch.tensor(b).cuda(),
                              tuple(dhw), precision=0)
    b2 = torch.full((N, 32, 2), float("nan"), device="cuda")
    H.check(lib.ddpm3d_gn_finalize(H.ptr(stats), co, stats.shape[2], 0, 0, 0, N, 32, float(T), 1e-5,
                                   0, 0, 0, 0, 0, 0, 0, H.ptr(b2), H.stream()))
    torch.cuda.synchronize()
    qkv = qkv.reshape(N, T, co)
    c = R.wiring_case(qkv.cpu().numpy(), b2.cpu().numpy(), heads, ch)
    print("wiring: the loosest entry is %.3gx, the largest entry %.3gx the sample's maximum"
          % (c.guarantees["loosest_entry"], c.guarantees["max_entry_looseness"]))
    _check(c, _run(c, precision, qkv_dev=qkv, bound_dev=b2), precision)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", [n for n in R.names("a") if n != "bound_8x_too_small"])
def test_bound_conventions(name, precision):
    """interleaved entries with the maximum in one entry and 1e30 in every other slot, 1 / 33 / 64 entries, bounds
    1x / 40x / 2^12 loose, a power-of-two bound and the float below one (the data reaches both), bound 0 on zeros
    (output exactly 0) and on O(1) data, bound inf, per-sample magnitudes (1, 2^-27), (2^-27, 1) and
    (1, 2^-27, 2^-10) with each sample's own entries -- the per (sample, head) figure makes the small sample count"""
    c = R.case(name)
    _check(c, _run(c, precision), precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_bound_too_small_is_loud_not_wrong(precision):
    """A bound 8x too small: in the f16x3 mode every output element is either non-finite or within the bar (and
    some are non-finite: f16 overflowed) -- never a finite wrong value; the exact mode ignores the bound."""
    c = R.case("bound_8x_too_small")
    got = _run(c, precision)
    ref = R.case_reference(c.name)
    if precision == 0:
        return _hold_to_the_bars(c, got, ref, precision)
    scale = np.abs(ref.reshape(c.N, c.T, c.heads, c.ch)).max(axis=(1, 3), keepdims=True)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - ref).reshape(c.N, c.T, c.heads, c.ch) <= R.BAR * scale
    finite = np.isfinite(got).reshape(ok.shape)
    print("attention (a) %s f16x3: %.3f of the outputs are finite" % (c.name, finite.mean()))
    assert (~finite | ok).all()
    assert not finite.all()


# ---------------------------------------------------------------------------------------------------------------
# (b) the recurrence
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", R.names("b"))
def test_softmax_recurrence(name, precision):
    """the running max rising in every tile (every rescale taken, l and the accumulators both scaled), falling
    (alpha == 1 from tile 1 on), rising for the even or for the odd queries of every wave (the f16x3 kernel
    decides the rescale per wave), the maximum at the last key of the ragged tile, all logits <= -10 beside
    zero-padded keys of score 0, identical keys (output = mean of v), and one-hot weights: there the exact mode
    returns the matching v row bit for bit and the f16x3 mode within 2^-21 |v| + 2^-24 max|v| per element"""
    c = R.case(name)
    _check(c, _run(c, precision), precision)


# ---------------------------------------------------------------------------------------------------------------
# (c) edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", [n for n in R.names("c") if n.startswith("edge_")])
def test_sequence_length_edges(name, precision):
    """T = 1, 2, 31 (one ragged tile), 32, 33, 127, 128, 129 (a second query block with one valid query and three
    waves with none), 257; N = 2, two heads, head 1's v 2^-12 of head 0's"""
    c = R.case(name)
    _check(c, _run(c, precision), precision)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", ["guard_T77", "guard_T129"])
def test_guard_rows(name, precision):
    """qkv and out are interiors of larger allocations with 128 guard rows on either side (16-byte aligned
    interior pointers).  qkv's guards are NaN and the output is finite and within the bars: nothing outside the
    tensor is read into the result.  out and its guards start as a sentinel: afterwards the guards are
    bit-identical and no sentinel is left inside."""
    import guided_diffusion._hip as H
    lib = H.load()
    c = R.case(name)
    assert c.N == 1
    C3, Co = c.heads * 3 * c.ch, c.heads * c.ch
    qbig = torch.full((c.T + 2 * GUARD, C3), float("nan"), device="cuda")
    qbig[GUARD:GUARD + c.T] = torch.tensor(c.qkv[0]).cuda()
    bd = torch.tensor(c.bound).cuda()
    qptr, outs = qbig.data_ptr() + GUARD * C3 * 4, []
    for _ in range(2):
        obig = torch.tensor(np.full((c.T + 2 * GUARD, Co), SENTINEL, np.int32).view(np.float32)).cuda()
        optr = obig.data_ptr() + GUARD * Co * 4
        assert qptr % 16 == 0 and optr % 16 == 0
        H.check(lib.ddpm3d_attention_p(qptr, 1, c.T, c.heads, c.ch, precision, bd.data_ptr() + 4 * c.offset, c.count,
                                       c.stride, optr, H.stream()))
        torch.cuda.synchronize()
        outs.append(obig.cpu().numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    bits = _bits(outs[0])
    assert (bits[:GUARD] == SENTINEL).all() and (bits[GUARD + c.T:] == SENTINEL).all()
    assert not (bits[GUARD:GUARD + c.T] == SENTINEL).any()
    _check(c, outs[0][GUARD:GUARD + c.T].reshape(1, c.T, Co), precision)


# ---------------------------------------------------------------------------------------------------------------
# (d) argument checks
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """Everything ddpm3d_attention_p refuses, with its code and ddpm3d_last_error() text; nothing launches (the
    NaN-filled output is untouched).  The exact mode takes a null bound through both entry points."""
    import guided_diffusion._hip as H
    lib = H.load()
    N, T, heads, ch = 1, 16, 1, 32
    qkv = torch.zeros(N, T + 1, heads * 3 * ch, device="cuda")
    out = torch.full((N, T + 1, heads * ch), float("nan"), device="cuda")
    bound = torch.ones(64, device="cuda")
    q, o, b = H.ptr(qkv), H.ptr(out), H.ptr(bound)

    def call(qp=q, n=N, t=T, h=heads, c=ch, prec=1, bp=b, count=1, stride=1, op=o):
        return lib.ddpm3d_attention_p(qp, n, t, h, c, prec, bp, count, stride, op, H.stream())

    def refused(rc, code, text):
        assert rc == code, (rc, code, text)
        assert text in lib.ddpm3d_last_error(), lib.ddpm3d_last_error()

    needs_bound = b"needs qkv_bound (1..64 entries per sample)"
    refused(call(bp=0), H.E_INVAL, needs_bound)
    for count in (0, 65, -1):
        refused(call(count=count), H.E_INVAL, needs_bound)
    for stride in (0, -2):
        refused(call(stride=stride), H.E_INVAL, needs_bound)
    for kw in (dict(n=0), dict(t=0), dict(h=0), dict(n=-1), dict(t=-1), dict(h=-1), dict(qp=0), dict(op=0)):
        for prec in (0, 1):
            refused(call(prec=prec, **kw), H.E_INVAL, b"attention: bad arguments")
    for prec in (0, 1):
        refused(call(qp=q + 4, prec=prec), H.E_INVAL, b"16-byte aligned")
        refused(call(op=o + 4, prec=prec), H.E_INVAL, b"16-byte aligned")
    for prec in (2, 3, 4, 5, 6):
        refused(call(prec=prec), H.E_NOSUP, b"attention: precision %d" % prec)
    for c in (16, 48, 256):
        refused(call(c=c), H.E_NOSUP, b"channels per head")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # the boundaries that are accepted: 1 and 64 entries, and no bound at all in the exact mode
    assert call(count=1) == 0 and call(count=64) == 0
    assert call(prec=0, bp=0, count=0, stride=0) == 0
    assert lib.ddpm3d_attention(q, N, T, heads, ch, o, H.stream()) == 0
    torch.cuda.synchronize()
    assert (out[:, :T] == 0).all() and torch.isnan(out[:, T]).all()
