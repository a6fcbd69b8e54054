"""
The attention core (csrc/attention.hip) on the CPU: an fp64 reference, the adversarial inputs of
test_gpu_attention.py, and a streaming fp64 model of the f16x3 kernel's operand arithmetic.

reference(qkv, heads, ch)   softmax((q s)(k s)^T) v, s = ch^-1/4, in fp64 on the channels-last layout the
                            kernel reads: qkv [N][T][heads*3*ch] (heads outermost, then q | k | v) ->
                            [N][T][heads*ch].
CASES / case(name)          the inputs: each builder returns a Case (qkv, the bound array with its
                            (offset, count, stride), what the case guarantees) and ASSERTS that guarantee in
                            fp64, so a case cannot silently stop being adversarial.
model(qkv, ..., mut=...)    the f16x3 kernel's arithmetic with exact products and fp64 sums: qkv_scale's rule,
                            the f16 hi/lo split (numpy's float16 cast), three partial products, 32-key tiles
                            with the running max / alpha / l recurrence, P split at x4096 relative to the
                            RUNNING max, the final 1/(l S 4096).  It hosts the mutations of MUTATIONS (the
                            plausible kernel bugs); it sets no bar.

Nothing here touches a GPU.
"""

import math
from dataclasses import dataclass, field

import numpy as np

KT = 32                 # keys per tile
WAVE = 32               # queries per wave
P_SCALE = 4096.0
BAR = 1e-5              # per (sample, head): max|got - ref| / max|ref|   (test_attention_core_vs_legacy_reference)
ROW_BAR = 1e-4          # per query row: max_c|err| / max_c|ref|          (the long-sequence test)

MUTATIONS = (
    "sample0_scale",            # sample 0's scale for every sample
    "first_entry_only",         # no max over the bound entries
    "ignore_stride",            # bound entries read at stride 1
    "ignore_offset",            # the other interleaved column is read
    "no_mask",                  # the ragged tile's padded keys keep score 0
    "no_rescale",               # alpha forced to 1 for oacc
    "no_l_rescale",             # alpha forced to 1 for l
    "rescale_by_first_query",   # the wave's rescale decision from its first query, not the ballot
    "drop_q_lo", "drop_k_lo", "drop_v_lo", "drop_p_lo",
    "scale_once",               # q scaled by ch^-1/4, not ch^-1/2
)


# ------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------
def _heads(qkv, heads, ch):
    x = np.asarray(qkv, dtype=np.float64)
    N, T, C3 = x.shape
    assert C3 == heads * 3 * ch
    x = x.reshape(N, T, heads, 3, ch)
    return x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2]          # q, k, v: [N][T][heads][ch]


def logits(qkv, heads, ch):
    """(q s)(k s)^T in fp64: [N][heads][T queries][T keys]"""
    q, k, _ = _heads(qkv, heads, ch)
    s = ch ** -0.25
    return np.einsum("nthc,nshc->nhts", q * s, k * s)


def reference(qkv, heads, ch):
    _, _, v = _heads(qkv, heads, ch)
    lg = logits(qkv, heads, ch)
    w = np.exp(lg - lg.max(axis=-1, keepdims=True))
    w /= w.sum(axis=-1, keepdims=True)
    N, T = v.shape[:2]
    return np.einsum("nhts,nshc->nthc", w, v).reshape(N, T, heads * ch)


def head_errors(got, ref, heads, ch):
    """(per (sample, head) figure [N][heads], per query row figure [N][T][heads]); a non-finite output is inf"""
    got = np.asarray(got, dtype=np.float64)
    N, T, _ = ref.shape
    g, r = got.reshape(N, T, heads, ch), np.asarray(ref, dtype=np.float64).reshape(N, T, heads, ch)
    with np.errstate(invalid="ignore"):
        e = np.abs(g - r)
    e = np.where(np.isfinite(g), e, np.inf)
    per_head = e.max(axis=(1, 3)) / np.maximum(np.abs(r).max(axis=(1, 3)), 1e-300)
    per_row = e.max(axis=3) / np.maximum(np.abs(r).max(axis=3), 1e-300)
    return per_head, per_row


# ------------------------------------------------------------------------------------------------------------
# the f16x3 kernel's arithmetic
# ------------------------------------------------------------------------------------------------------------
def scale_exponent(b):
    """qkv_scale's k: S = 2^k, k = 14 - floor(log2 b) from the exponent field, 0 for b <= 0 / inf / NaN,
    clamped to +-40"""
    b = np.float32(b)
    e = int((b.view(np.uint32) >> np.uint32(23)) & np.uint32(0xff)) - 127
    k = 14 - e
    if not (b > 0) or e == 128:
        k = 0
    return max(-40, min(40, k))


def qkv_scale(bound, offset, count, stride, n, mut=()):
    """sample n's power-of-two scale from the bound array: the max (fmaxf: a NaN entry is dropped) over the
    `count` entries at bound[offset + (n * count + i) * stride]"""
    bound = np.asarray(bound, dtype=np.float32).ravel()
    if "sample0_scale" in mut:
        n = 0
    if "ignore_offset" in mut and stride > 1:
        offset = (offset + 1) % stride
    if "ignore_stride" in mut:
        stride = 1
    entries = bound[offset + (n * count + np.arange(count)) * stride]
    if "first_entry_only" in mut:
        entries = entries[:1]
    b = np.fmax.reduce(np.concatenate([np.zeros(1, np.float32), entries]))
    return 2.0 ** scale_exponent(b)


def _split(x32, S, drop_lo=False):
    """split_f16: s = x * S in fp32, hi = f16(s), lo = f16(s - hi); returned as fp64"""
    with np.errstate(all="ignore"):
        s = np.asarray(x32, dtype=np.float32) * np.float32(S)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    if drop_lo:
        lo = np.zeros_like(lo)
    return hi, lo


def model(qkv, heads, ch, bound, offset, count, stride, mut=()):
    """The f16x3 kernel's operand arithmetic, streaming, products exact and sums in fp64.  mut: a name or a
    collection of names from MUTATIONS."""
    mut = {mut} if isinstance(mut, str) else set(mut)
    assert mut <= set(MUTATIONS), mut
    x = np.asarray(qkv, dtype=np.float32)
    N, T, _ = x.shape
    x = x.reshape(N, T, heads, 3, ch)
    out = np.empty((N, T, heads, ch))
    qs = np.float32(ch ** -0.25) if "scale_once" in mut else np.float32(1.0) / np.sqrt(np.float32(ch))
    first = (np.arange(T) // WAVE) * WAVE                   # each query's wave's first query
    with np.errstate(all="ignore"):
        for n in range(N):
            S = qkv_scale(bound, offset, count, stride, n, mut)
            for h in range(heads):
                qh, ql = _split(x[n, :, h, 0] * qs, S, "drop_q_lo" in mut)
                m = np.full(T, -np.inf)
                l = np.zeros(T)
                o = np.zeros((T, ch))
                for k0 in range(0, T, KT):
                    nv = min(KT, T - k0)
                    kt, vt = np.zeros((KT, ch), np.float32), np.zeros((KT, ch), np.float32)   # keys beyond T are zeros
                    kt[:nv], vt[:nv] = x[n, k0:k0 + nv, h, 1], x[n, k0:k0 + nv, h, 2]
                    kh, kl = _split(kt, S, "drop_k_lo" in mut)
                    vh, vl = _split(vt, S, "drop_v_lo" in mut)
                    sacc = qh @ kl.T + ql @ kh.T + qh @ kh.T                   # [T][KT], x S^2
                    if nv < KT and "no_mask" not in mut:
                        sacc[:, nv:] = -np.inf
                    lg = sacc / (S * S)
                    m_new = np.fmax(m, np.fmax.reduce(lg, axis=1))
                    alpha = np.exp(m - m_new)                                  # first tile: exp(-inf) = 0
                    p = np.exp(lg - m_new[:, None])
                    l = l * (1.0 if "no_l_rescale" in mut else alpha) + p.sum(axis=1)
                    ps = (p * P_SCALE).astype(np.float32)
                    ph = ps.astype(np.float16)
                    pl = (ps - ph.astype(np.float32)).astype(np.float16).astype(np.float64)
                    ph = ph.astype(np.float64)
                    if "drop_p_lo" in mut:
                        pl = np.zeros_like(pl)
                    a_o = alpha
                    if "no_rescale" in mut:
                        a_o = np.ones(T)
                    elif "rescale_by_first_query" in mut:
                        a_o = np.where(alpha[first] != 1.0, alpha, 1.0)
                    o = o * a_o[:, None] + (ph @ vl + pl @ vh + ph @ vh)
                    m = m_new
                out[n, :, h] = o / (l * S * P_SCALE)[:, None]
    return out.reshape(N, T, heads * ch)


# ------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str                  # "a" bound conventions, "b" the recurrence, "c" edges
    heads: int
    ch: int
    qkv: np.ndarray             # float32 [N][T][heads*3*ch]
    bound: np.ndarray           # float32, flat: what the bound pointer's allocation holds
    offset: int                 # floats between the allocation's start and the pointer the kernel gets
    count: int
    stride: int
    kind: str = "bar"           # "bar": the two bars | "zero": exactly 0 | "loud": non-finite or within the bar |
                                # "onehot": the element bound of the one-hot case
    match: np.ndarray = None    # one-hot: [N][heads][T] the key each query selects
    guarantees: dict = field(default_factory=dict)

    @property
    def N(self):
        return self.qkv.shape[0]

    @property
    def T(self):
        return self.qkv.shape[1]


def _assemble(q, k, v):
    """q, k, v [N][T][heads][ch] -> float32 qkv [N][T][heads*3*ch]"""
    x = np.stack([q, k, v], axis=3)
    N, T = x.shape[:2]
    return np.ascontiguousarray(x.reshape(N, T, -1).astype(np.float32))


def _gauss(N, T, heads, ch, seed, mags=None):
    g = np.random.default_rng(seed)
    x = g.standard_normal((N, T, heads * 3 * ch))
    if mags is not None:
        x = x * np.asarray(mags, dtype=np.float64).reshape(N, 1, 1)
    return np.ascontiguousarray(x.astype(np.float32))


def _absmax(qkv):
    return np.abs(qkv).reshape(qkv.shape[0], -1).max(axis=1).astype(np.float32)


def _lay_out(entries, offset, stride, fill):
    """entries [N][count] at fill-ed array[offset + (n * count + i) * stride]"""
    entries = np.asarray(entries, dtype=np.float32)
    N, count = entries.shape
    assert 0 <= offset < stride
    arr = np.full(N * count * stride, fill, dtype=np.float32)
    arr[offset + np.arange(N * count) * stride] = entries.ravel()
    return arr


def _exact_bound(qkv):
    return dict(bound=_absmax(qkv), offset=0, count=1, stride=1)


def _peaked_entries(name, group, heads, ch, T, N, count, stride, offset, pos, seed):
    """the true maximum in entry `pos` only, every other entry 2^-30 of it, every other slot 1e30"""
    qkv = _gauss(N, T, heads, ch, seed, mags=[1.0, 0.25, 3.0][:N])
    mx = _absmax(qkv)
    entries = np.repeat((mx * np.float32(2.0 ** -30))[:, None], count, axis=1)
    entries[:, pos] = mx
    arr = _lay_out(entries, offset, stride, 1e30)
    # guarantee: the max of a sample's entries is the true maximum and sits in `pos` alone
    got = arr[offset + np.arange(N * count) * stride].reshape(N, count)
    assert (got.argmax(axis=1) == pos % count).all() and (got.max(axis=1) == mx).all()
    assert (np.delete(got, pos % count, axis=1) <= mx[:, None] * 2.0 ** -30).all() or count == 1
    assert stride == 1 or (np.delete(arr, offset + np.arange(N * count) * stride) == np.float32(1e30)).all()
    return Case(name, group, heads, ch, qkv, arr, offset, count, stride,
                guarantees=dict(max_entry=pos % count, others=2.0 ** -30))


def _loose(name, ch, factor, seed):
    qkv = _gauss(2, 96, 2, ch, seed)
    b = (_absmax(qkv).astype(np.float64) * factor).astype(np.float32)
    assert (b >= _absmax(qkv)).all()
    return Case(name, "a", 2, ch, qkv, b, 0, 1, 1, guarantees=dict(loose=factor))


def _mantissa(name, ch, b, seed):
    """the bound is exactly b and the data reaches it"""
    b = np.float32(b)
    g = np.random.default_rng(seed).standard_normal((1, 77, 2 * 3 * ch))
    x = (g * (float(b) / np.abs(g).max())).astype(np.float32)
    i = np.unravel_index(np.abs(g).argmax(), g.shape)
    x = np.clip(x, -b, b)
    x[i] = np.copysign(b, g[i])
    assert np.abs(x).max() == b
    return Case(name, "a", 2, ch, x, np.array([b], np.float32), 0, 1, 1,
                guarantees=dict(bound_bits=hex(int(b.view(np.uint32)))))


def _per_sample(name, ch, mags, wiring, seed):
    N = len(mags)
    qkv = _gauss(N, 70, 2, ch, seed, mags=mags)
    mx = _absmax(qkv)
    assert all(mx[n] >= np.abs(qkv[n]).max() for n in range(N))
    ratios = mx.astype(np.float64) / mx.max()
    assert ratios.min() < 2.0 ** -25                      # the gap that makes a wrong sample's scale visible
    if wiring:
        arr = _lay_out(np.repeat(mx[:, None], 32, axis=1), 1, 2, 1e30)
        return Case(name, "a", 2, ch, qkv, arr, 1, 32, 2, guarantees=dict(mags=mags))
    return Case(name, "a", 2, ch, qkv, mx, 0, 1, 1, guarantees=dict(mags=mags))


def _directional(N, T, heads, ch, seed, sign_of_query, levels):
    """q_t = +-4 ch^1/4 u + noise, k_j = ch^1/4 levels[j] u + noise with a unit vector u: the logit of (t, j) is
    +-4 levels[j] plus O(0.1) noise"""
    g = np.random.default_rng(seed)
    c4 = ch ** 0.25
    q, k = np.empty((N, T, heads, ch)), np.empty((N, T, heads, ch))
    for n in range(N):
        for h in range(heads):
            u = g.choice([-1.0, 1.0], ch) / math.sqrt(ch)
            A = 4.0 * c4 * np.asarray(sign_of_query, dtype=np.float64)
            q[n, :, h] = A[:, None] * u + 0.05 * g.standard_normal((T, ch))
            k[n, :, h] = (c4 * levels)[:, None] * u + 0.05 * g.standard_normal((T, ch))
    v = g.standard_normal((N, T, heads, ch))
    return _assemble(q, k, v)


def _tile_maxima(lg):
    """[..., T queries, tiles]: the largest logit of each 32-key tile"""
    T = lg.shape[-1]
    return np.stack([lg[..., k0:k0 + KT].max(axis=-1) for k0 in range(0, T, KT)], axis=-1)


def _assert_rising(tm):
    """every tile raises the running max"""
    run = np.maximum.accumulate(tm, axis=-1)
    assert (tm[..., 1:] > run[..., :-1]).all()


def _assert_falling(tm):
    """the max sits in tile 0: alpha == 1 from tile 1 on"""
    assert (tm[..., 1:] < tm[..., :1]).all()


def _ramp(name, ch, T, kind, seed, heads=2):
    """rising: the logit rises with the key index for every query (from -15 to +15 over the T keys: with the
    logits inside +-16 the slope is 30 / T per key, and every 32-key tile raises every query's max by 32 slopes);
    falling: it falls; even / odd: the even (odd) queries rise and the others fall, inside every wave"""
    t = np.arange(T)
    sign = {"rising": np.ones(T), "falling": -np.ones(T), "even": np.where(t % 2 == 0, 1.0, -1.0),
            "odd": np.where(t % 2 == 1, 1.0, -1.0)}[kind]
    qkv = _directional(1, T, heads, ch, seed, sign, np.linspace(-3.7, 3.7, T))
    lg = logits(qkv, heads, ch)
    assert np.abs(lg).max() <= 16.0
    tm = _tile_maxima(lg)
    assert tm.shape[-1] >= 2
    _assert_rising(tm[:, :, sign > 0])
    if (sign < 0).any():
        _assert_falling(tm[:, :, sign < 0])
    rise = float(np.diff(tm[:, :, sign > 0], axis=-1).min()) if (sign > 0).any() else None
    return Case(name, "b", heads, ch, qkv, **_exact_bound(qkv), guarantees=dict(kind=kind, min_tile_rise=rise))


def _tail_max(name, ch, T, seed):
    """the largest logit of every query at the last key, in the ragged tile"""
    g = np.random.default_rng(seed)
    heads, c4 = 2, ch ** 0.25
    q, k = np.empty((1, T, heads, ch)), np.empty((1, T, heads, ch))
    for h in range(heads):
        u = g.choice([-1.0, 1.0], ch) / math.sqrt(ch)
        q[0, :, h] = 4.0 * c4 * u + 0.5 * g.standard_normal((T, ch))
        k[0, :, h] = 0.5 * g.standard_normal((T, ch))
        k[0, T - 1, h] = 2.5 * c4 * u
    qkv = _assemble(q, k, g.standard_normal((1, T, heads, ch)))
    lg = logits(qkv, heads, ch)
    assert T % KT and (lg.argmax(axis=-1) == T - 1).all() and np.abs(lg).max() <= 16.0
    margin = float((lg[..., T - 1] - lg[..., :T - 1].max(axis=-1)).min())
    assert margin > 2.0
    return Case(name, "b", heads, ch, qkv, **_exact_bound(qkv), guarantees=dict(margin=margin))


def _all_negative(name, ch, T, seed):
    """q ~ +a, k ~ -a: every logit in [-16, -10]; an unmasked padded key (score 0) would take nearly all the weight"""
    g = np.random.default_rng(seed)
    heads = 2
    a = math.sqrt(12.7 / math.sqrt(ch))
    q = a + 0.15 * g.standard_normal((1, T, heads, ch))
    k = -a + 0.15 * g.standard_normal((1, T, heads, ch))
    qkv = _assemble(q, k, g.standard_normal((1, T, heads, ch)))
    lg = logits(qkv, heads, ch)
    assert T % KT and lg.max() <= -10.0 and lg.min() >= -16.0
    # the weight 32 - T % 32 unmasked keys of score 0 would take from a query
    pad = KT - T % KT
    stolen = pad / (pad + np.exp(lg).sum(axis=-1))
    assert stolen.min() > 0.999
    return Case(name, "b", heads, ch, qkv, **_exact_bound(qkv),
                guarantees=dict(logit_range=(float(lg.min()), float(lg.max())), stolen=float(stolen.min())))


def _uniform(name, ch, T, seed):
    """all keys identical: the output is the mean of v"""
    g = np.random.default_rng(seed)
    heads = 2
    q = g.standard_normal((1, T, heads, ch))
    k = np.repeat(g.standard_normal((1, 1, heads, ch)), T, axis=1)
    v = g.standard_normal((1, T, heads, ch))
    qkv = _assemble(q, k, v)
    ref = reference(qkv, heads, ch)
    mean = np.repeat(_heads(qkv, heads, ch)[2].mean(axis=1, keepdims=True), T, axis=1).reshape(1, T, heads * ch)
    assert np.abs(ref - mean).max() <= 1e-12
    return Case(name, "b", heads, ch, qkv, **_exact_bound(qkv), guarantees=dict(output="mean of v"))


def _hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def _one_hot(name, ch, T, seed):
    """q_t = a c_pi(t), k_j = a c_j with +-1 codes (the rows of the ch x ch Hadamard matrix and their negatives:
    c_i . c_j is 0 or -ch): the matching logit a^2 sqrt(ch) = 114 exceeds every other by >= 110, so every other
    weight, and alpha across the jump, underflow to exactly 0 in fp32 (exp(-110) < the smallest denormal)"""
    assert ch < T <= 2 * ch or T <= ch
    g = np.random.default_rng(seed)
    heads = 2
    Hm = _hadamard(ch)
    codes = np.concatenate([Hm, -Hm])[:T]
    a = math.sqrt(114.0 / math.sqrt(ch))
    q, k = np.empty((1, T, heads, ch)), np.empty((1, T, heads, ch))
    match = np.empty((1, heads, T), dtype=np.int64)
    for h in range(heads):
        pi = g.permutation(T)
        match[0, h] = pi
        q[0, :, h] = a * codes[pi]
        k[0, :, h] = a * codes
    v = g.standard_normal((1, T, heads, ch))
    qkv = _assemble(q, k, v)
    lg = logits(qkv, heads, ch)
    hit = np.take_along_axis(lg, match[..., None], axis=-1)[..., 0]
    rest = lg.copy()
    np.put_along_axis(rest, match[..., None], -np.inf, axis=-1)
    gap = float((hit - rest.max(axis=-1)).min())
    assert gap >= 110.0
    tiles = (T + KT - 1) // KT
    for h in range(heads):
        for w0 in range(0, T, WAVE):                 # each full wave of queries has matches in first and last tile
            seen = set(match[0, h, w0:w0 + WAVE] // KT)
            assert len(match[0, h, w0:w0 + WAVE]) < WAVE or {0, tiles - 1} <= seen
        assert set(match[0, h] // KT) == set(range(tiles))       # first, every middle and the ragged last tile
    assert T % KT
    return Case(name, "b", heads, ch, qkv, **_exact_bound(qkv), kind="onehot", match=match,
                guarantees=dict(gap=gap, tiles=tiles))


def one_hot_expected(c):
    """(the v row each query selects [N][T][heads*ch], the element bound 2^-21 |v| + 2^-24 max|v| of the f16x3
    mode: the split's representation error and one final rounding; max|v| per (sample, head))"""
    _, _, v = _heads(c.qkv, c.heads, c.ch)
    N, T = v.shape[:2]
    sel = np.empty_like(v)
    for n in range(N):
        for h in range(c.heads):
            sel[n, :, h] = v[n, c.match[n, h], h]
    bound = 2.0 ** -21 * np.abs(sel) + 2.0 ** -24 * np.abs(v).max(axis=(1, 3), keepdims=True)
    return sel.reshape(N, T, -1), bound.reshape(N, T, -1)


def _edge(T, ch):
    """Gaussian, N = 2, heads = 2; head 1's v is 2^-12 of head 0's, so only a per-head figure sees head 1"""
    x = _gauss(2, T, 2, ch, 300 + T).reshape(2, T, 2, 3, ch)
    x[:, :, 1, 2] *= np.float32(2.0 ** -12)
    qkv = np.ascontiguousarray(x.reshape(2, T, -1))
    v = _heads(qkv, 2, ch)[2]
    r = np.abs(v[:, :, 1]).max() / np.abs(v[:, :, 0]).max()
    assert r < 2.0 ** -10
    return Case("edge_T%d" % T, "c", 2, ch, qkv, **_exact_bound(qkv), guarantees=dict(v_ratio=float(r)))


def wiring_qkv_inputs(heads=2, ch=32, cin=64, dhw=(3, 6, 6), seed=90):
    """inputs of the 1x1 qkv conv of the network-wiring case (T = 108: three full key tiles and a ragged one):
    x [N][cin][D][H][W] with sample 1 a thousandth of sample 0, w [heads*3*ch][cin][1][1][1], bias"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((2, cin) + tuple(dhw)).astype(np.float32)
    x[1] *= np.float32(1e-3)
    co = heads * 3 * ch
    w = (g.standard_normal((co, cin, 1, 1, 1)) / math.sqrt(cin)).astype(np.float32)
    w *= np.linspace(0.05, 1.5, co, dtype=np.float32).reshape(co, 1, 1, 1, 1)     # groups of unlike magnitude
    return x, w, np.zeros(co, np.float32)              # no bias: sample 1's qkv stays a thousandth of sample 0's


def wiring_case(qkv, bounds2, heads, ch, name="wiring"):
    """The network's convention (unet_plan.hip, engine.py): bounds2 = the bounds-only gn_finalize output
    [N][32][2], the kernel gets (pointer + 1 float, 32, 2).  Asserts that each of the 32 entries read bounds the
    true |qkv| of its group of channels."""
    qkv = np.ascontiguousarray(np.asarray(qkv, dtype=np.float32))
    b2 = np.asarray(bounds2, dtype=np.float32)
    N, T, C3 = qkv.shape
    assert b2.shape == (N, 32, 2) and C3 % 32 == 0
    true = np.abs(qkv).reshape(N, T, 32, C3 // 32).max(axis=(1, 3))
    assert (b2[:, :, 1] >= true * (1 - 1e-6)).all()
    loosest = float((b2[:, :, 1] / true).max())
    return Case(name, "a", heads, ch, qkv, b2.ravel().copy(), 1, 32, 2,
                guarantees=dict(loosest_entry=loosest, max_entry_looseness=float((b2[:, :, 1].max(axis=1) / true.max(axis=1)).max())))


def _wiring_like(seed=91):
    """the CPU tier's stand-in for the wiring case: the same conv evaluated on the CPU, per-group bounds between
    1x and 40x loose (what test_gn_finalize_bounds_are_upper_bounds allows), the other column 1e30"""
    heads, ch = 2, 32
    x, w, b = wiring_qkv_inputs(heads, ch)
    N, cin = x.shape[:2]
    y = np.einsum("nct,oc->nto", x.reshape(N, cin, -1).astype(np.float64), w.reshape(-1, cin).astype(np.float64)) + b
    qkv = y.astype(np.float32)
    g = np.random.default_rng(seed)
    true = np.abs(qkv).reshape(N, qkv.shape[1], 32, -1).max(axis=(1, 3))
    loose = g.uniform(1.0, 40.0, true.shape)
    loose[:, 7] = 40.0
    b2 = np.stack([np.full_like(true, 1e30), true * loose], axis=-1).astype(np.float32)
    return wiring_case(qkv, b2, heads, ch, name="wiring_like")


def _builders():
    B = {}
    group = None

    def add(name, fn):
        nonlocal group
        assert name not in B
        B[name] = fn
        GROUP[name] = group

    # (a) bound conventions
    group = "a"
    add("wiring_like", _wiring_like)
    add("entries32_max_last", lambda: _peaked_entries("entries32_max_last", "a", 2, 32, 77, 2, 32, 2, 1, 31, 101))
    add("entries32_max_first", lambda: _peaked_entries("entries32_max_first", "a", 2, 64, 77, 2, 32, 2, 1, 0, 102))
    add("entries1", lambda: _peaked_entries("entries1", "a", 1, 128, 45, 2, 1, 2, 1, 0, 103))
    add("entries33_max_last", lambda: _peaked_entries("entries33_max_last", "a", 2, 32, 45, 2, 33, 3, 2, 32, 104))
    add("entries64_max_last", lambda: _peaked_entries("entries64_max_last", "a", 2, 64, 45, 3, 64, 1, 0, 63, 105))
    add("loose_x1", lambda: _loose("loose_x1", 32, 1.0, 110))
    add("loose_x40", lambda: _loose("loose_x40", 64, 40.0, 111))
    add("loose_x4096", lambda: _loose("loose_x4096", 128, 4096.0, 112))
    add("bound_power_of_two", lambda: _mantissa("bound_power_of_two", 64, 4.0, 120))
    add("bound_ulp_below_power_of_two",
        lambda: _mantissa("bound_ulp_below_power_of_two", 128, np.nextafter(np.float32(4.0), np.float32(0.0)), 121))

    def zero_zero():
        qkv = np.zeros((2, 45, 2 * 3 * 32), np.float32)
        return Case("bound0_zero_data", "a", 2, 32, qkv, np.zeros(2, np.float32), 0, 1, 1, kind="zero")

    def degenerate(name, ch, b, seed):
        qkv = _gauss(2, 77, 2, ch, seed)
        return Case(name, "a", 2, ch, qkv, np.full(2, b, np.float32), 0, 1, 1, guarantees=dict(S=1.0))

    add("bound0_zero_data", zero_zero)
    add("bound0_unit_data", lambda: degenerate("bound0_unit_data", 64, 0.0, 130))
    add("bound_inf_unit_data", lambda: degenerate("bound_inf_unit_data", 128, np.inf, 131))

    def too_small():
        qkv = _gauss(2, 77, 2, 32, 140)
        b = _absmax(qkv) / np.float32(8.0)
        return Case("bound_8x_too_small", "a", 2, 32, qkv, b, 0, 1, 1, kind="loud", guarantees=dict(understated=8.0))

    add("bound_8x_too_small", too_small)
    add("samples_1_tiny", lambda: _per_sample("samples_1_tiny", 32, (1.0, 2.0 ** -27), True, 150))
    add("samples_tiny_1", lambda: _per_sample("samples_tiny_1", 64, (2.0 ** -27, 1.0), True, 151))
    add("samples_1_tiny_small", lambda: _per_sample("samples_1_tiny_small", 128, (1.0, 2.0 ** -27, 2.0 ** -10), False, 152))

    # (b) the recurrence
    group = "b"
    add("rising_T160", lambda: _ramp("rising_T160", 32, 160, "rising", 200))
    add("rising_T300", lambda: _ramp("rising_T300", 128, 300, "rising", 201))
    add("rising_T61", lambda: _ramp("rising_T61", 64, 61, "rising", 206))      # 0.49 per key, second tile ragged
    add("falling_T160", lambda: _ramp("falling_T160", 64, 160, "falling", 202))
    add("mixed_even_rising", lambda: _ramp("mixed_even_rising", 64, 200, "even", 203))
    add("mixed_odd_rising", lambda: _ramp("mixed_odd_rising", 32, 200, "odd", 204))
    add("mixed_even_rising_ch128", lambda: _ramp("mixed_even_rising_ch128", 128, 130, "even", 205, heads=1))
    add("tail_max_T77", lambda: _tail_max("tail_max_T77", 64, 77, 210))
    add("all_negative_T77", lambda: _all_negative("all_negative_T77", 32, 77, 220))
    add("all_negative_T45", lambda: _all_negative("all_negative_T45", 128, 45, 221))
    add("all_negative_T77_ch64", lambda: _all_negative("all_negative_T77_ch64", 64, 77, 222))
    add("uniform_T100", lambda: _uniform("uniform_T100", 64, 100, 230))
    add("one_hot_T109", lambda: _one_hot("one_hot_T109", 128, 109, 240))
    add("one_hot_T77", lambda: _one_hot("one_hot_T77", 64, 77, 241))
    add("one_hot_T45", lambda: _one_hot("one_hot_T45", 32, 45, 242))

    # (c) edges
    group = "c"
    for T, ch in [(1, 32), (2, 64), (31, 128), (32, 32), (33, 64), (127, 128), (128, 32), (129, 64), (257, 128)]:
        add("edge_T%d" % T, lambda T=T, ch=ch: _edge(T, ch))

    def guard(name, T, heads, ch, seed):
        qkv = _gauss(1, T, heads, ch, seed)
        return Case(name, "c", heads, ch, qkv, **_exact_bound(qkv))

    add("guard_T77", lambda: guard("guard_T77", 77, 2, 32, 310))
    add("guard_T129", lambda: guard("guard_T129", 129, 1, 128, 311))
    return B


GROUP = {}                          # name -> "a" | "b" | "c", known without building a case
_BUILDERS = _builders()
CASES = tuple(_BUILDERS)            # the names
_BUILT = {}


def case(name):
    """the built (and self-checked) case; built once, shared, never modified"""
    if name not in _BUILT:
        c = _BUILDERS[name]()
        assert c.name == name and c.group == GROUP[name]
        c.qkv.setflags(write=False)
        c.bound.setflags(write=False)
        _BUILT[name] = c
    return _BUILT[name]


_REFS = {}


def case_reference(name):
    if name not in _REFS:
        c = case(name)
        r = reference(c.qkv, c.heads, c.ch)
        r.setflags(write=False)
        _REFS[name] = r
    return _REFS[name]


def names(group):
    return [n for n in CASES if GROUP[n] == group]
