"""
fp64 restatement of the timestep-conditioning path (reference nn.py:103-121 timestep_embedding, unet.py:464-478 time_embed
and label_emb, :703-705 emb = time_embed(.) + label_emb(y), :178-186 / :245-257 every ResBlock's emb_layers) and what its
tests share: their cases, their inputs, their bars and their comparator (tests/test_gpu_cond.py runs them against the
kernels, tests/test_cond_ref_cpu.py against the MUTANTS below).  Written from the cited lines; imports nothing of the
package.  `u` = 2^-24 throughout, the relative error of one fp32 rounding.

Bars, per element, nothing excluded; an element the kernel leaves unwritten (NaN) or a NaN where the reference has a
number is an infinite excess:

  timestep embedding   one fp32 ulp of the reference (ulp_bar), and at most EMB_FLIP_CAP elements of the whole test not
      bit-equal.  args = t * freqs is ONE fp32 product of two fp32 numbers (nn.py:117, freqs being the fp32 host table of
      :114-116), the same on every IEEE machine; cos / sin of it are evaluated in fp64 and rounded once, which is the
      correctly rounded fp32 value unless the fp64 result lies within the evaluation's own error (about 2^-52 relative)
      of an fp32 rounding midpoint (2^-25 relative): a chance of about 2^-27 per element, 1.6 million elements.

  linear   |got - (sum_k s_k w_k + b)| <= gamma_m (1 + 5u [silu]) (sum_k |s_k w_k| + |b|) + 5u sum_k |s_k w_k| [silu]
      with gamma_m = m u / (1 - m u) and m = ceil(K / 64) + 6 + 1 (linear_bar).  The kernel gives output o one wave; lane
      l runs acc = fmaf(s_k, w_k, acc) over k = l, l + 64, ... -- at most ceil(K / 64) fused operations of one rounding
      each (the first, onto acc = 0, rounds the product) --, then wave_sum: for (o = 32; o > 0; o >>= 1) v += shfl_xor(v,
      o), six additions on every value's way to lane 0, then s + bias[o], one more.  Every product therefore passes
      through at most m roundings and the bias through one (Higham, Accuracy and Stability, 3.1: any order of summation
      with at most m roundings on each term's path obeys the gamma_m bound).  SiLU-in: the kernel evaluates s =
      x / (1 + expf(-x)).  expf is within 1 ulp <= 2u relative (HIP's math API table, the figure
      tests/test_gpu_step_edges.py relies on); e' = e (1 + d1), |d1| <= 2u; 1 + e' rounds once: (1 + e')(1 + d2); the
      IEEE divide once more.  (1 + e') = (1 + e)(1 + d1 e / (1 + e)) and e / (1 + e) <= 1, so the denominator is off by
      at most 2u + u and s by 3u + u = 4u to first order; 5u covers the second-order terms (16 u^2 << u).  The products
      the gamma_m term multiplies are formed from the kernel's s, hence the (1 + 5u).  Valid where nothing overflows or
      goes subnormal: |x| <= 80 (expf(80) = 5.5e34); the tails beyond that have a test of their own.

  label embedding   bit-equal to the one fp32 add emb + table[y]; rows with a label outside [0, num_classes) bit-equal
      to what they held.

  film_rows, stage by stage   the bars above, each stage's reference evaluated from the previous stage's fp32 values.
  film_rows, end to end   B_next = |W| (1.1 B_prev) + linear_bar, from B = one ulp of the embedding; |silu'| <= 1.0998
      < 1.1 carries an input's error through the SiLU (and 1 <= 1.1 through the Linear without one); the label add
      contributes one rounding, u |emb + table[y]|.  The same recurrence with the worst case of an unknown fp32
      summation order, gamma_{K+1} (sum |s_k w_k| + |b|), and the same 5u for its SiLU, bounds the reference
      implementation's own fp32 run, whose recorded outputs are tests/golden/cond.npz (film_rows(..., arith="torch")).
"""

import math

import numpy as np
import torch

F = np.float32
U = 2.0 ** -24
LIN_ROWS = 8                  # rows one workgroup of the linear kernel handles
LANES = 64
WAVE_SUM_ADDS = 6             # ops.hip wave_sum: o = 32, 16, 8, 4, 2, 1
EMB_FLIP_CAP = 2              # elements of the whole embedding test that may differ from the reference (by one ulp)
NAN = float("nan")


# =============================================================================================== timestep embedding
def freq_table(dim, shift=0):
    """nn.py:114-116: the fp32 host table, by torch's fp32 exp as the reference evaluates it.  shift = 1: the table an
    index off by one would read, continued by the same formula."""
    half = dim // 2
    return torch.exp(-math.log(10000) * torch.arange(start=shift, end=half + shift, dtype=torch.float32) / half).numpy()


def _cos_sin(args, longdouble=False):
    a = args.astype(np.longdouble if longdouble else np.float64)
    return np.cos(a).astype(F), np.sin(a).astype(F)


def timestep_embedding(t, dim, freqs, mut=None, longdouble=False):
    """t [rows] fp32, freqs [dim // 2] fp32 -> [rows, dim] fp32: [cos | sin] of the fp32 product, a zero column behind
    an odd dim."""
    t = np.asarray(t)
    assert t.dtype == F and freqs.dtype == F and freqs.shape == (dim // 2,)
    if mut == "emb_freq_off_by_one":
        freqs = freq_table(dim, shift=1)
    if mut == "emb_args_fp64":
        args = t.astype(np.float64)[:, None] * freqs.astype(np.float64)[None]
    else:
        args = t[:, None] * freqs[None]                       # one fp32 rounding, nn.py:117
        assert args.dtype == F
    c, s = _cos_sin(args, longdouble)
    if mut == "emb_cos_sin_swapped":
        c, s = s, c
    out = np.concatenate([c, s], axis=1)                      # :118
    if dim % 2:                                               # :119-120
        out = np.concatenate([out, np.full((len(t), 1), 1.0 if mut == "emb_pad_not_zero" else 0.0, F)], axis=1)
    return out


def ulp_bar(ref):
    return np.spacing(np.abs(ref.astype(F))).astype(np.float64)


# ========================================================================================================== linear
def silu64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def linear(x, w, b, silu_in, mut=None):
    """x [rows, K], w [O, K], b [O] fp32 -> fp64 value [rows, O] and sumabs = sum_k |s_k w_k|."""
    assert x.dtype == F and w.dtype == F and b.dtype == F
    rows, K = x.shape
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    silu = bool(silu_in)
    if mut == "lin_silu_flipped":
        silu = not silu
    if silu:
        if mut == "lin_fast_silu":                            # exp with 2^-21 relative error
            s = x64 / (1.0 + np.exp(-x64) * (1.0 + 2.0 ** -21))
        else:
            s = silu64(x64)
    else:
        s = x64
    if mut == "lin_row_mod_8":
        s = s[np.arange(rows) % LIN_ROWS]
    if mut == "lin_row_0":
        s = s[np.zeros(rows, dtype=np.int64)]
    if mut == "lin_tail_chunk_dropped":
        s, w64 = s[:, :K // LANES * LANES], w64[:, :K // LANES * LANES]
    if mut == "lin_bias_off_by_one":
        b64 = np.roll(b64, -1)
    return s @ w64.T + b64[None], np.abs(s) @ np.abs(w64).T


def gamma(m):
    return m * U / (1.0 - m * U)


def linear_roundings(K):
    return -(-K // LANES) + WAVE_SUM_ADDS + 1


def linear_bar(x, w, b, silu_in):
    """The kernel's per-element bound (module docstring)."""
    _, sumabs = linear(x, w, b, silu_in)
    absb = np.abs(b.astype(np.float64))[None]
    g = gamma(linear_roundings(x.shape[1]))
    if silu_in:
        return g * (1.0 + 5 * U) * (sumabs + absb) + 5 * U * sumabs
    return g * (sumabs + absb)


def torch_linear_bar(x, w, b, silu_in):
    """An fp32 Linear of unknown summation order: K products, K additions with the bias in any order, gamma_{K+1}."""
    _, sumabs = linear(x, w, b, silu_in)
    absb = np.abs(b.astype(np.float64))[None]
    g = gamma(x.shape[1] + 1)
    if silu_in:
        return g * (1.0 + 5 * U) * (sumabs + absb) + 5 * U * sumabs
    return g * (sumabs + absb)


def place(val, out_stride, mut=None):
    """What the output buffer holds after the launch: [rows, out_stride] NaN-filled fp32 with row r's O values at
    r * out_stride."""
    rows, O = val.shape
    buf = np.full(rows * out_stride, NAN, F)
    stride = O if mut == "lin_out_stride_ignored" else out_stride
    with np.errstate(over="ignore", invalid="ignore"):
        v32 = val.astype(F)
    for r in range(rows):
        buf[r * stride:r * stride + O] = v32[r]
    return buf.reshape(rows, out_stride)


def excess(got, ref, bar):
    """max |got - ref| / bar over all elements; inf where exactly one of the two is NaN or where a difference meets a
    zero bar.  ref's NaNs (the gap columns of a strided output) must be NaN in got."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    if (gn != rn).any():
        return math.inf
    d = np.abs(np.where(rn, 0.0, got) - np.where(rn, 0.0, ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bar)
    return float(q.max()) if q.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------- label embedding
def add_embedding(emb, table, y, mut=None):
    """emb [rows, dim] fp32, table [num_classes, dim] fp32, y [rows] int64 -> emb + table[y] in one fp32 add; a label
    outside [0, num_classes) leaves its row as it was (ops.hip: the kernel's own promise)."""
    assert emb.dtype == F and table.dtype == F
    y = np.asarray(y, dtype=np.int64)
    nc = table.shape[0]
    if mut == "lab_row_off_by_one":
        y = y + 1
    if mut == "lab_out_of_range_clamped":
        y = np.clip(y, 0, nc - 1)
    ok = (y >= 0) & (y < nc)
    out = emb.copy()
    out[ok] = emb[ok] + table[y[ok]]
    return out


# ====================================================================================================== the path
def res_prefixes(topo):
    """state_dict prefixes of the ResBlocks in the engine's layer order: input blocks, middle block, output blocks."""
    return [e.prefix for e in topo.all_layers() if e.kind == "res"]


def fused_emb_layers(params, topo, film, mut=None):
    """[film_total, 4 mc] weight and [film_total] bias of every ResBlock's emb_layers.1, back to back in layer order,
    and each block's offset.  Additive variant (film False: h = conv1(.) + emb_out, unet.py:256-257): conv1's bias
    rides on the Linear's, one fp32 add."""
    ws, bs, off, total = [], [], {}, 0
    for i, p in enumerate(res_prefixes(topo)):
        w = np.asarray(params[p + ".emb_layers.1.weight"], dtype=F)
        b = np.asarray(params[p + ".emb_layers.1.bias"], dtype=F)
        if not film and mut != "film_no_conv_bias_fold":
            b = b + np.asarray(params[p + ".in_layers.2.bias"], dtype=F)
        if mut == "film_off_shifted" and i == 1:              # one block's scale and shift halves change places
            h = w.shape[0] // 2
            w, b = np.concatenate([w[h:], w[:h]]), np.concatenate([b[h:], b[:h]])
        off[p] = total
        total += w.shape[0]
        ws.append(w)
        bs.append(b)
    return np.concatenate(ws), np.concatenate(bs), off


def conv_bias_fold(params, topo):
    """Additive variant: the first convs' biases, back to back in layer order (what the engine's row carries beyond
    emb_layers' output), and the one fp32 rounding of folding them into the Linear's bias, u |b + conv bias|."""
    cb = np.concatenate([np.asarray(params[p + ".in_layers.2.bias"], dtype=F) for p in res_prefixes(topo)])
    b = np.concatenate([np.asarray(params[p + ".emb_layers.1.bias"], dtype=F) for p in res_prefixes(topo)])
    return cb.astype(np.float64), U * np.abs((b + cb).astype(np.float64))


def film_rows(params, topo, t, y=None, film=True, mut=None, arith="kernel"):
    """The whole path in fp64 from a state_dict of fp32 numpy arrays.  -> dict of fp64 arrays temb, e1, e2 (after the
    label add), rows, and `bound`: the propagated bound of rows, `bound_e2` that of e2, for the arithmetic `arith`
    ("kernel": linear_bar; "torch": an fp32 run of unknown summation order)."""
    bar_of = linear_bar if arith == "kernel" else torch_linear_bar
    P = {k: np.asarray(params[k], dtype=F) for k in ("time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight",
                                                     "time_embed.2.bias")}
    mc = P["time_embed.0.weight"].shape[1]
    t = np.asarray(t, dtype=F)
    temb = timestep_embedding(t, mc, freq_table(mc))
    B = ulp_bar(temb)

    def stage(x64, B, w, b, silu):
        x32 = x64.astype(F)          # the fp64 chain itself is carried in fp64; bars are evaluated at its fp32 image
        if silu:
            val = silu64(x64) @ w.astype(np.float64).T + b.astype(np.float64)[None]
        else:
            val = x64 @ w.astype(np.float64).T + b.astype(np.float64)[None]
        return val, (1.1 * B) @ np.abs(w.astype(np.float64)).T + bar_of(x32, w, b, silu)

    e1, B = stage(temb.astype(np.float64), B, P["time_embed.0.weight"], P["time_embed.0.bias"], 0)
    e2, B = stage(e1, B, P["time_embed.2.weight"], P["time_embed.2.bias"], 1)
    if y is not None:
        table = np.asarray(params["label_emb.weight"], dtype=F).astype(np.float64)
        yy = np.asarray(y, dtype=np.int64)
        if mut == "lab_row_off_by_one":
            yy = (yy + 1) % table.shape[0]
        e2 = e2 + table[yy]
        B = B + U * np.abs(e2)
    w, b, off = fused_emb_layers(params, topo, film, mut)
    rows, Brows = stage(e2, B, w, b, 1)
    return dict(temb=temb.astype(np.float64), e1=e1, e2=e2, rows=rows, bound=Brows, bound_e2=B, off=off)


# =========================================================================================================== cases
def emb_times(kind):
    """fp32 timesteps of an embedding case."""
    if kind == "ints":                                        # every index of a 1000-step process
        return np.arange(1000, dtype=F)
    if kind == "mixed":                                       # 1000 rows: rescaled and fractional ones
        a = [k * (1000.0 / 250) for k in range(250)]          # rescale_timesteps on the "250" table
        b = [k * (1000.0 / 7) for k in range(28)]             # fractional, up to 3857 (a 4000-step schedule)
        c = [3999.0, 0.0]
        d = [0.25 * (5 * k + 1) for k in range(720)]          # 4000 steps rescaled to [0, 1000): quarters
        return np.array(a + b + c + d, dtype=F)
    if kind == "five":
        return np.array([0.0, 3999.0, 1000.0 / 7, 6000.0 / 7, 996.0], dtype=F)
    if kind == "one":
        return np.array([3000.0 / 7], dtype=F)
    raise KeyError(kind)


EMB_CASES = [dict(name="emb_d%d_%s" % (dim, kind), dim=dim, kind=kind)
             for dim in (2, 6, 32, 128, 129, 512) for kind in ("one", "five", "ints", "mixed")]

# (rows, K, O): every value of each axis, and each neighbouring pair around 8 rows, 64 columns, 4 outputs
LIN_SHAPES = [(1, 1, 1), (7, 63, 3), (8, 64, 4), (9, 65, 5), (17, 100, 70), (1000, 128, 514), (1, 512, 514),
              (8, 63, 4), (9, 64, 3), (7, 65, 4), (8, 65, 3), (9, 63, 5), (17, 128, 1), (1000, 512, 3), (1, 100, 4),
              (7, 1, 70), (9, 512, 70), (17, 64, 5), (8, 128, 3), (1000, 65, 5), (7, 64, 5), (9, 100, 4)]
LIN_CASES = [dict(name="lin_r%d_k%d_o%d_%s" % (r, K, O, "silu" if s else "id"), rows=r, K=K, O=O, silu=s)
             for r, K, O in LIN_SHAPES for s in (0, 1)]
SMALL = 1e-5                  # scale of the one small output column
GAP = 3                       # out_stride = O + GAP in the strided launches


def lin_inputs(case):
    """x ~ 2 N(0, 1) (|x| < 80), w ~ 0.05 N, b ~ 0.1 N; column O // 2 (weights and bias) scaled by 1e-5."""
    rows, K, O = case["rows"], case["K"], case["O"]
    g = np.random.default_rng([rows, K, O, case["silu"]])
    x = (2.0 * g.standard_normal((rows, K))).astype(F)
    w = (0.05 * g.standard_normal((O, K))).astype(F)
    b = (0.1 * g.standard_normal(O)).astype(F)
    small = O // 2
    w[small] *= F(SMALL)
    b[small] *= F(SMALL)
    assert np.abs(x).max() < 80
    return x, w, b, small


LAB_CASES = [dict(name="lab_r%d_d%d_c%d" % (r, d, c), rows=r, dim=d, nc=c)
             for r in (1, 5, 300) for d in (1, 7, 512) for c in (1, 10)]
BAD_LABELS = (-1, None, 2 ** 40)          # None: num_classes itself


def lab_launches(case):
    """-> list of (emb, table, y): one launch for the 5- and 300-row cases, one per label for the 1-row case."""
    rows, dim, nc = case["rows"], case["dim"], case["nc"]
    g = np.random.default_rng([rows, dim, nc])
    emb = g.standard_normal((rows, dim)).astype(F)
    table = g.standard_normal((nc, dim)).astype(F)
    special = [0, nc - 1] + [nc if v is None else v for v in BAD_LABELS]
    if rows == 1:
        return [(emb, table, np.array([v], dtype=np.int64)) for v in special]
    y = g.integers(0, nc, rows)
    y[:5] = special
    if rows > 5:
        y[-3:] = special[2:]                                  # the bad ones again, in the last block
    return [(emb, table, y.astype(np.int64))]


# ------------------------------------------------------------------------------------------------------ film cases
PUBLISHED = dict(large_size=96, small_size=96, num_channels=128, num_res_blocks=2, num_head_channels=64,
                 attention_resolutions="1000", learn_sigma=True, resblock_updown=True, use_scale_shift_norm=True)
TINY = dict(PUBLISHED, num_channels=32, num_res_blocks=1)
MODELS = {                    # tag: (factory flags, seed of the synthetic parameters)
    "tiny": (TINY, 0),
    "tiny_additive": (dict(TINY, use_scale_shift_norm=False), 0),
    "tiny_class_cond": (dict(TINY, class_cond=True), 4),
    "published": (PUBLISHED, 0),
}
SCHEDULES = {                 # tag: (diffusion steps, respacing, rescale_timesteps)
    "250": (1000, "250", False),
    "250_rescaled": (1000, "250", True),
    "10": (1000, "10", False),
}
FILM_CASES = [dict(name="%s_%s" % (m, s), model=m, sched=s, film=MODELS[m][0]["use_scale_shift_norm"],
                   class_cond=bool(MODELS[m][0].get("class_cond")))
              for m in MODELS for s in SCHEDULES]
# the golden's timesteps: 0, 999, integers between, and fractional rescaled ones (a 4000-step process rescaled to
# [0, 1000) gives quarters; k * 1000 / 7 a 7-step one); GOLDEN_ROWS[tag] leading entries are recorded per model
GOLDEN_T = np.array([0.0, 999.0, 250.25, 1000.0 / 7, 37.0, 499.0, 500.75, 6000.0 / 7, 4.0, 996.0, 1.0, 3999.0], dtype=F)
GOLDEN_ROWS = {"tiny": 12, "tiny_additive": 12, "tiny_class_cond": 12, "published": 7}
GOLDEN_SEED_Y = 77


def golden_labels(rows, num_classes=1000):
    y = np.random.default_rng(GOLDEN_SEED_Y).integers(0, num_classes, rows)
    y[0], y[1] = 0, num_classes - 1
    return y.astype(np.int64)


def cond_params(keys_and_shapes, seed, synth_param):
    """fp32 numpy parameters of the path from a state_dict's (key, shape) pairs and the synthetic-weight recipe"""
    return {k: synth_param(k, tuple(s), seed) for k, s in cond_keys(keys_and_shapes)}


def cond_keys(keys_and_shapes):
    """the entries of a state_dict the conditioning path reads"""
    return [(k, s) for k, s in keys_and_shapes
            if k.startswith("time_embed.") or k.startswith("label_emb.") or ".emb_layers.1." in k
            or k.endswith(".in_layers.2.bias")]


# ========================================================================================================= mutants
# name -> the stage whose cases have to see it.  A mutant that cannot change a case's result (the pad column of an even
# dim, the tail chunk where K is a multiple of 64, ...) is named in IDENTITY with the condition; everywhere else the
# comparator must see it at ten times the bar.
MUTANTS = {
    "emb_cos_sin_swapped": "emb",
    "emb_freq_off_by_one": "emb",
    "emb_args_fp64": "emb",
    "emb_pad_not_zero": "emb",
    "lin_tail_chunk_dropped": "lin",
    "lin_row_mod_8": "lin",
    "lin_row_0": "lin",
    "lin_silu_flipped": "lin",
    "lin_bias_off_by_one": "lin",
    "lin_fast_silu": "silu_probe",
    "lin_out_stride_ignored": "lin_strided",
    "lab_row_off_by_one": "lab",
    "lab_out_of_range_clamped": "lab",
    "film_off_shifted": "film",
    "film_no_conv_bias_fold": "film",
}
IDENTITY = {
    # dim 2 has the one frequency 1.0: t * 1.0 is exact in either precision
    "emb_args_fp64": lambda c: c["dim"] == 2,
    "emb_pad_not_zero": lambda c: c["dim"] % 2 == 0,
    "lin_tail_chunk_dropped": lambda c: c["K"] % LANES == 0,
    "lin_row_mod_8": lambda c: c["rows"] <= LIN_ROWS,
    "lin_row_0": lambda c: c["rows"] == 1,
    "lin_bias_off_by_one": lambda c: c["O"] == 1,
    "lin_out_stride_ignored": lambda c: c["rows"] == 1,
    "film_no_conv_bias_fold": lambda c: c["film"],
}

# The SiLU probe.  linear_bar cannot see an exp of 2^-21 relative error: that is 8u in s at most, and the bar of the
# shortest chain (K = 1: m = 8) is already (8 + 5) u.  With K = 1, w = 1 and b = 0 every operation after the SiLU is
# exact (fmaf(s, 1, 0) = s, wave_sum adds zeros, s + 0), so the output IS the kernel's s and is held to the SiLU term
# alone, 5u |silu(x)|.  The mutant's error is 8u e / (1 + e) |silu(x)|, e = exp(-x): above the bar for x < -0.52,
# below ten times the bar for every x, which no bar that admits a 1-ulp expf can change (8u < 10 * 4u).  The mutant
# test therefore asks of this one mutant that it exceeds the bar, not ten times the bar.
SILU_PROBE_X = np.concatenate([np.linspace(-80, 80, 641), [-0.5, 0.5, -1e-3, 1e-3, -20.0, -10.0, -5.0]]).astype(F)


def silu_probe_ref(mut=None):
    x = SILU_PROBE_X[:, None]
    val, _ = linear(x, np.ones((1, 1), F), np.zeros(1, F), 1, mut)
    return val, 5 * U * np.abs(silu64(x))
