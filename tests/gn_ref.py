"""
fp64 reference of the GroupNorm statistics chain (numpy only, no GPU):

    statistics rows [N][C][rows][2] fp64  ->  ddpm3d_gn_finalize (ops.hip: gn_finalize_kernel)  ->  A, B, bound

finalize_ref follows the kernel step by step with every fp32 rounding left out, finalize_bars bounds what those
roundings (and the kernel's own order of the fp64 row sums) can move, Mut switches in the plausible bugs, and
gnacc_sums / delta emulate and bound the conv epilogues' pivoted fp32 accumulation (conv3d_params.h: GnAcc), from
which the contract of `bound` follows: a bound of max |x| up to the relative slack delta(n).
"""

from dataclasses import dataclass

import numpy as np

U32 = 2.0 ** -24      # unit roundoff of fp32 (round to nearest)
U64 = 2.0 ** -53
TINY32 = 2.0 ** -149  # one rounding in fp32's subnormal range


@dataclass
class Mut:
    """plausible bugs of gn_finalize_kernel (all off = the kernel as written)"""
    rows0_for_src1: bool = False      # rows0 used as the second source's row count
    drop_last_pass: bool = False      # the load loop stops before a last, partial pass of 8 x blockDim items
    film_sample0: bool = False        # sample 0's FiLM row for every sample
    film_off_ignored: bool = False    # film_off taken as 0
    shift_half: bool = False          # the shift row read at C // 2 behind the scale row's start (not at C)
    count_no_cg: bool = False         # count not multiplied by the group's width
    no_eps: bool = False              # rstd = 1 / sqrt(var)
    max_over_sums: bool = False       # the row maximum taken over the sums, not over the sums of squares
    group_from_src0: bool = False     # a group that starts in source 1 read from source 0


def partition(rng, total, rows, empty=0.1):
    """row lengths: `rows` non-negative integers that add up to `total`, uneven, about `empty` of them zero
    (never the first or the last: a run's ends must show when they are missed)"""
    w = rng.random(rows) + 0.05
    w[rng.random(rows) < empty] = 0.0
    w[0] = w[-1] = 1.0
    edges = np.floor(np.cumsum(w) / w.sum() * total + 0.5).astype(np.int64)
    edges[-1] = total
    return np.diff(np.concatenate([[0], edges]))


def make_stats(x, row_lengths):
    """fp64 [N][C][rows][2] (sum, sum of squares) of an fp32 [N][C][voxels] array over consecutive runs of
    row_lengths[r] voxels (any partition of the voxels: uneven rows, empty rows = (0, 0))"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    L = np.asarray(row_lengths, dtype=np.int64)
    assert (L >= 0).all() and L.sum() == x.shape[2]
    xd = x.astype(np.float64)
    st = np.zeros(x.shape[:2] + (len(L), 2))
    live = np.nonzero(L)[0]
    starts = (np.cumsum(L) - L)[live]
    st[:, :, live, 0] = np.add.reduceat(xd, starts, axis=2)
    st[:, :, live, 1] = np.add.reduceat(xd * xd, starts, axis=2)
    return st


def launch_threads(C0, rows0, C1, rows1, groups):
    """ddpm3d_launch_gn_finalize: 1024 threads from 2048 items of the LONGER side on"""
    return 1024 if max(rows0, rows1) * ((C0 + C1) // groups) >= 2048 else 256


def _runs(st0, st1, groups, mut):
    """per (n, g): the run of (sum, sumsq) pairs the kernel folds, as it addresses them (flat, zeros past the end
    of the buffer: what the kernel's bounded buffer loads return at worst under a mutation)"""
    N, C0, rows0 = st0.shape[:3]
    C1, rows1 = (st1.shape[1], st1.shape[2]) if st1 is not None else (0, 0)
    C = C0 + C1
    cg = C // groups
    threads = launch_threads(C0, rows0, C1, rows1, groups)
    flat = [st0.reshape(-1, 2), st1.reshape(-1, 2) if st1 is not None else None]
    out = []
    for n in range(N):
        for g in range(groups):
            cbeg = g * cg
            from0 = cbeg < C0
            cs = cbeg if from0 else cbeg - C0
            if mut.group_from_src0:
                from0 = True
            Cs, rows = (C0, rows0) if from0 else (C1, rows0 if mut.rows0_for_src1 else rows1)
            items = rows * cg
            start = (n * Cs + cs) * rows
            run = flat[0 if from0 else 1][start:start + items]
            if mut.drop_last_pass:
                run = run[:items // (threads * 8) * (threads * 8)]
            out.append(run)
    return out, N, C, cg


def _film_rows(film, film_stride, film_off, N, C, mut):
    """(scale, shift) [N][C] fp64 as the kernel indexes them"""
    f = np.asarray(film, dtype=np.float64).reshape(-1)
    off = 0 if mut.film_off_ignored else film_off
    sc = np.empty((N, C))
    sh = np.empty((N, C))
    for n in range(N):
        base = (0 if mut.film_sample0 else n) * film_stride + off
        sc[n] = f[base:base + C]
        s0 = base + (C // 2 if mut.shift_half else C)
        sh[n] = f[s0:s0 + C]
    return sc, sh


def finalize_ref(st0, st1, count, eps, gamma, beta, film, film_stride, film_off, groups, mut=None):
    """gn_finalize_kernel in fp64, step by step: per (n, g) fold the group's run of rows (sums in extended
    precision), xmax = sqrt(largest row sum of squares) (NaN rows ignored, like fmaxf), mean, clamped variance,
    rstd with eps AS THE KERNEL GETS IT (a float), a = rstd gamma, b = beta - mean a, FiLM a (1 + sc),
    b (1 + sc) + sh, and entry 0 of the bound max|a| xmax + max|b| (NaNs ignored).  gamma None: bounds only.
    Returns dict(A, B [N][C]; xmax, bound0 [N][groups]; s1, s2, abs1, abs2, items [N][groups]; mean, var, rstd)."""
    mut = mut or Mut()
    runs, N, C, cg = _runs(st0, st1, groups, mut)
    G = groups
    s1 = np.empty((N, G)); s2 = np.empty((N, G)); a1 = np.empty((N, G)); a2 = np.empty((N, G))
    items = np.empty((N, G)); m2 = np.empty((N, G))
    for i, run in enumerate(runs):
        n, g = divmod(i, G)
        ld = run.astype(np.longdouble)
        s1[n, g] = float(ld[:, 0].sum()); s2[n, g] = float(ld[:, 1].sum())
        a1[n, g] = float(np.abs(ld[:, 0]).sum()); a2[n, g] = float(np.abs(ld[:, 1]).sum())
        items[n, g] = len(run)
        col = run[:, 0] if mut.max_over_sums else run[:, 1]
        m2[n, g] = np.fmax.reduce(col, initial=0.0) if len(col) else 0.0
    with np.errstate(all="ignore"):
        xmax = np.sqrt(m2)
        r = dict(xmax=xmax, s1=s1, s2=s2, abs1=a1, abs2=a2, items=items, A=None, B=None,
                 bound0=xmax.copy())
        if gamma is None:
            return r
        cnt = float(count) * (1 if mut.count_no_cg else cg)
        mean = s1 / cnt
        var = s2 / cnt - mean * mean
        var = np.where(var < 0.0, 0.0, var)
        e = 0.0 if mut.no_eps else float(np.float32(eps))
        rstd = 1.0 / np.sqrt(var + e)
        rep = lambda v: np.repeat(v, cg, axis=1)
        gm = np.asarray(gamma, dtype=np.float64)[None, :]
        bt = np.asarray(beta, dtype=np.float64)[None, :]
        A = rep(rstd) * gm
        B = bt - rep(mean) * A
        if film is not None:
            sc, sh = _film_rows(film, film_stride, film_off, N, C, mut)
            A = A * (1.0 + sc)
            B = B * (1.0 + sc) + sh
        amax = np.fmax.reduce(np.abs(A).reshape(N, G, cg), axis=2, initial=0.0)
        bmax = np.fmax.reduce(np.abs(B).reshape(N, G, cg), axis=2, initial=0.0)
        r.update(A=A, B=B, bound0=amax * xmax + bmax, mean=mean, var=var, rstd=rstd, cnt=cnt, eps=e)
    return r


def finalize_bars(st0, st1, count, eps, gamma, beta, film, film_stride, film_off, groups):
    """Per-element bounds (barA, barB), each [N][C], on |A_kernel - A64| and |B_kernel - B64|, u = 2^-24, v = 2^-53.
    Every term is a worst case (no statistics), first-order products carried in full:

      (1) order of the fp64 row sums: the kernel adds a group's `items` rows per thread, wave and workgroup in an
          order of its own; any order of n additions is within n v sum|terms| of the exact sum:
              e1 = items v sum|row sums|,  e2 = items v sum|row sums of squares|
      (2) mean = s1 / cnt:   dmean = e1 / cnt + v |mean|
      (3) the variance's cancellation: var = s2 / cnt - mean^2 rounds the quotient, the square and the
          difference at the size of the OPERANDS, not of var:
              dvar = e2 / cnt + (2 |mean| + dmean) dmean + 3 v (|s2| / cnt + mean^2)
          (the clamp at zero moves nothing further: it is 1-Lipschitz)
      (4) rstd: 1 / sqrt is monotone, so the kernel's fp64 value lies between 1 / sqrt(var + dvar + eps) and
          1 / sqrt(max(var - dvar, 0) + eps), plus 3 v for sqrt, quotient and the sum; ONE fp32 rounding of rstd
      (5) meanf = (float) mean: one fp32 rounding
      (6) a = rstd * gamma: the product's rounding;  b = fmaf(-meanf, a, beta): one rounding of the exact
          -meanf a + beta
      (7) FiLM: sc = 1 + scale rounds once; a * sc and fmaf(b, sc, sh) one more each
      (8) 2^-149 per rounding for results in fp32's subnormal range.
    NaN where the reference is NaN (a NaN row)."""
    r = finalize_ref(st0, st1, count, eps, gamma, beta, film, film_stride, film_off, groups)
    N, G = r["s1"].shape
    cg = r["A"].shape[1] // G
    cnt = r["cnt"]
    u, v = U32, U64
    rnd = lambda val, err: err + u * (np.abs(val) + err) + TINY32          # one fp32 rounding of a value known to err
    prod = lambda x, dx, y, dy: np.abs(x) * dy + np.abs(y) * dx + dx * dy    # error of a product of two such values
    with np.errstate(all="ignore"):
        e1 = r["items"] * v * r["abs1"]
        e2 = r["items"] * v * r["abs2"]
        mean, var, e = r["mean"], r["var"], r["eps"]
        dmean = e1 / cnt + v * np.abs(mean)
        dvar = e2 / cnt + (2 * np.abs(mean) + dmean) * dmean + 3 * v * (np.abs(r["s2"]) / cnt + mean * mean)
        hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + e)
        lo = 1.0 / np.sqrt(var + dvar + e)
        rstd = r["rstd"]
        drstd = rnd(rstd, np.maximum(hi - rstd, rstd - lo) + 3 * v * rstd)
        dmeanf = rnd(mean, dmean)
        rep = lambda t: np.repeat(t, cg, axis=1)
        gm = np.asarray(gamma, dtype=np.float64)[None, :]
        bt = np.asarray(beta, dtype=np.float64)[None, :]
        a = rep(rstd) * gm
        da = rnd(a, np.abs(gm) * rep(drstd))
        b = bt - rep(mean) * a
        db = rnd(b, prod(rep(mean), rep(dmeanf), a, da))
        if film is not None:
            sc, _ = _film_rows(film, film_stride, film_off, N, a.shape[1], Mut())
            s = 1.0 + sc
            ds = rnd(s, 0.0)
            a, da = a * s, rnd(a * s, prod(a, da, s, ds))
            db = rnd(r["B"], prod(b, db, s, ds))
    return da, db


# --------------------------------------------------------------------------- GnAcc (conv3d_params.h)
def gnacc_sums(x, bug=None):
    """struct GnAcc on lanes x [L][n] (fp32): pivot p = the lane's first value, fp32 s1 = sum (x - p),
    s2 = fmaf(d, d, s2), ONE conversion in fp64: sum x = n p + s1, sum x^2 = s2 + 2 p s1 + n p^2.
    Returns (sum1, sum2) fp64 [L].  (fmaf is emulated as the fp32 rounding of the fp64 d*d + s2: d*d is exact in
    fp64, the double rounding differs from fmaf's single one in rare ties by one fp32 ulp of s2.)
    bug: "cross" = the conversion's 2 p s1 taken once, "count" = n - 1 pivots in n p^2, "pivot0" = sums around the
    pivot but converted as if it were 0 (what the test of the real writers must catch)."""
    x = np.asarray(x, dtype=np.float32)
    L, n = x.shape
    p = x[:, 0].copy()
    s1 = np.zeros(L, dtype=np.float32)
    s2 = np.zeros(L, dtype=np.float32)
    for i in range(n):
        d = (x[:, i] - p).astype(np.float32)
        s1 = (s1 + d).astype(np.float32)
        dd = d.astype(np.float64)
        s2 = (dd * dd + s2.astype(np.float64)).astype(np.float32)
    dp = p.astype(np.float64)
    if bug == "pivot0":
        return s1.astype(np.float64), s2.astype(np.float64)
    cross, cnt = (1.0 if bug == "cross" else 2.0), (n - 1 if bug == "count" else n)
    return n * dp + s1.astype(np.float64), s2.astype(np.float64) + cross * dp * s1.astype(np.float64) + cnt * dp * dp


def sum2_slack(n):
    """relative bound on |sum2 - sum x^2| of a GnAcc lane of n values, and so of any fp64 fold of such lanes
    (delta's docstring: gamma_(n+2) (3 (n - 1) + 2 sqrt(n - 1)) + eps64)"""
    n = int(n)
    if n <= 1:
        return U64 * 32
    g = (n + 2) * U32 / (1.0 - (n + 2) * U32)
    return float(g * (3.0 * (n - 1) + 2.0 * np.sqrt(n - 1.0)) + U64 * (16 * n + 16))


def delta(n):
    """Guaranteed relative shortfall: for a statistics row made of GnAcc lanes of at most n values each (folded in
    fp64), gn_finalize's  sqrtf((float) largest row sum2) >= max|x| (1 - delta(n)).

    Derivation, reading the struct (u = 2^-24, gamma_k = k u / (1 - k u), M = max|x_i|, T = sum x_i^2 >= M^2 of
    one lane, a_i = |x_i - p|, a_1 = 0):
      d_i = fl(x_i - p) = (x_i - p)(1 + e_i), |e_i| <= u.  s1 is a recursive fp32 sum of n terms, s2 a recursive
      fmaf chain, so  s1 = sum (x_i - p)(1 + eta_i),  s2 = sum (x_i - p)^2 (1 + psi_i)  with  |eta_i| <= gamma_n,
      |psi_i| <= gamma_(n+2)  (Higham, Accuracy and Stability, 3.1 / 4.2).  The conversion is exact algebra in
      fp64:  sum2 - T = sum a_i^2 psi_i + 2 p sum (x_i - p) eta_i, hence
          |sum2 - T| <= gamma_(n+2) (sum a_i^2 + 2 |p| sum a_i)
                      = gamma_(n+2) (sum_(i>=2) (a_i + |p|)^2 - (n - 1) p^2)
                     <= gamma_(n+2) (sum_(i>=2) (|x_i| + 2 |p|)^2 - (n - 1) p^2)
                      = gamma_(n+2) ((T - p^2) + 4 |p| sum_(i>=2) |x_i| + 3 (n - 1) p^2).
      With p^2 = t T, t in [0, 1], and Cauchy-Schwarz sum_(i>=2) |x_i| <= sqrt((n - 1)(T - p^2)):
          <= gamma_(n+2) T ((1 - t) + 4 sqrt((n - 1) t (1 - t)) + 3 (n - 1) t)
          <= gamma_(n+2) T (3 (n - 1) + 2 sqrt(n - 1))                    (n >= 2; sqrt(t (1 - t)) <= 1/2)
      -- attained to first order by the pivot being the one hot value of a flat lane (t -> 1): the PET lesion.
      The fp64 conversion and the fp64 fold of lanes into a row round ~ n + 8 times at 2^-53 of terms <= 4 n T:
      eps64 = 2^-53 (16 n + 16).  So every lane has sum2 >= T (1 - eps), eps = gamma_(n+2) (3 (n - 1) +
      2 sqrt(n - 1)) + eps64, a row's sum (of non-negative lane values) at least its hottest lane's, and
          sqrt(row sum2) >= M sqrt(1 - eps).
      gn_finalize then rounds three times in fp32 -- (float) sum2, sqrtf, and entry 0's fmaf -- each monotone,
      (1 - u) at worst; the square root halves the first:  delta(n) = 1 - sqrt(1 - eps) + 3 u.
      n = 1: d = 0, sum2 = p^2 exactly: only the 3 u remain.
    (Assumes M^2 above fp32's subnormal range, where fmaf(d, d, s2) can lose a whole square.)"""
    if int(n) <= 1:
        return 3 * U32
    return float(1.0 - np.sqrt(1.0 - sum2_slack(n)) + 3 * U32)


# the activation scale (conv3d_load.h: act_scale_finish) puts the BOUND b at b 2^k in [2^14, 2^15); a value that
# exceeds the bound by 1 / (1 - delta) lands below 2^15 / (1 - delta), and its f16 hi part rounds up by at most
# 1 + 2^-11: finite as long as  2^15 (1 + 2^-11) / (1 - delta) <= 65504
F16_MAX = 65504.0
def headroom_ok(d):
    return 2.0 ** 15 * (1.0 + 2.0 ** -11) / (1.0 - d) <= F16_MAX
