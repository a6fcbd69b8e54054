"""
numpy restatement of one p_sample / ddim_sample step (reference gaussian_diffusion.py:232-326, :395-439, :537-585), one
fp32 rounding at a time, and what the step kernel's edge tests share: their cases, their inputs and their comparator
(tests/test_gpu_step_edges.py runs them against the kernel, tests/test_step_ref_cpu.py against mutants of `step`).

Every arithmetic operation below is one np.float32 operation in the order of the reference's torch expressions, which
is the order the kernel's line-number comments cite; nothing is fused.  exp(0.5 * logvar) is evaluated in float64 from
the fp32 argument and rounded once (the correctly rounded fp32 value).  Coefficients come from
oracle/schedule_ref.spaced_schedule in fp64 and are cast to fp32 per use, as _extract_into_tensor(...).float() does
(:897-910); the package's coef_table() is not read.  The clip is np.clip, which keeps NaN as torch.clamp does.
Written from the cited lines' arithmetic; imports nothing of the package.
"""

import functools

import numpy as np

from oracle import schedule_ref

F = np.float32
U = 2.0 ** -24                       # half an ulp of 1.0f: the relative rounding error of one fp32 operation
STRIDE = 1024 * 256                  # voxels one pass of the step kernels' grid-stride loop covers (step_grid)


@functools.lru_cache(maxsize=None)
def schedule(respacing):
    """fp64 tables of linear-1000 respaced to `respacing` ("" = unspaced)"""
    return schedule_ref.spaced_schedule(1000, "linear", respacing)[1]


class Ops:
    """The places where a step kernel can go wrong, one method each; a mutant overrides one of them."""

    def rows(self, t):
        """the table row each sample reads"""
        return t

    def mask_rows(self, rows):
        """the row index each sample's t != 0 noise mask is taken from"""
        return rows

    def clip(self, x0):
        return np.clip(x0, F(-1), F(1))                               # :296-297, NaN stays NaN

    def posterior_mean(self, c1, x0, c2, x):
        return c1 * x0 + c2 * x                                       # :216-219

    def one_minus_ratio(self, ab, ab_prev):
        return F(1) - ab / ab_prev                                    # :573

    def variance_half(self, mo, n):
        """sample n's second half of the model output"""
        return mo[n, 1]

    def direction(self, ab_prev, sigma):
        return np.sqrt(F(1) - ab_prev - sigma * sigma)                # :579


OPS = Ops()


def _exp_r(a):
    return np.exp(a.astype(np.float64)).astype(F)


def step(kind, respacing, mo, x, z, t, learn_sigma, predict_xstart, clip, eta=0.0, xstart=None, sigma_small=False,
         ops=OPS):
    """One step of `kind` ("ddpm" or "ddim") for N samples: mo (N, 2 or 1, voxels), x, z, xstart (N, voxels) fp32,
    t one step index per sample.  `xstart`: a finished x0 used instead of the model output's first half (the _x0
    entries), clipped under `clip`.  -> fp32 arrays sample, pred_xstart, mean, log_variance, and noise_term, the
    (mask * sigma) * z that the step adds (what the DDPM bar is relative to)."""
    tb = schedule(respacing)
    N, voxels = x.shape
    assert mo.shape == (N, 2 if learn_sigma else 1, voxels) and z.shape == x.shape
    assert mo.dtype == x.dtype == z.dtype == F
    t = np.asarray(t, dtype=np.int64)
    assert t.shape == (N,) and t.min() >= 0 and t.max() < len(tb["betas"])
    rows = ops.rows(t)

    def c(table):
        return np.asarray(table, dtype=np.float64)[rows].astype(F)[:, None]

    with np.errstate(all="ignore"):
        c_recip, c_recipm1 = c(tb["sqrt_recip_alphas_cumprod"]), c(tb["sqrt_recipm1_alphas_cumprod"])
        if xstart is not None:
            x0 = xstart
        elif predict_xstart:
            x0 = mo[:, 0]                                             # :305-306
        else:
            x0 = c_recip * x - c_recipm1 * mo[:, 0]                   # :328-333
        if clip:
            x0 = ops.clip(x0)
        if learn_sigma:
            v = np.stack([ops.variance_half(mo, n) for n in range(N)])
            min_log, max_log = c(tb["posterior_log_variance_clipped"]), c(np.log(tb["betas"]))
            frac = (v + F(1)) / F(2)                                  # :274
            logvar = frac * max_log + (F(1) - frac) * min_log         # :275
        elif sigma_small:
            logvar = np.broadcast_to(c(tb["posterior_log_variance_clipped"]), x.shape)
        else:
            logvar = np.broadcast_to(c(np.log(np.append(tb["posterior_variance"][1], tb["betas"][1:]))), x.shape)
        mean = ops.posterior_mean(c(tb["posterior_mean_coef1"]), x0, c(tb["posterior_mean_coef2"]), x)
        mask = (ops.mask_rows(rows) != 0).astype(F)[:, None]          # :434-436, :581-583
        if kind == "ddpm":
            term = mask * _exp_r(F(0.5) * logvar) * z
            sample = mean + term                                      # :438
        else:
            eps = (c_recip * x - x0) / c_recipm1                      # :566, :345-349
            ab, ab_prev = c(tb["alphas_cumprod"]), c(tb["alphas_cumprod_prev"])
            sigma = F(eta) * np.sqrt((F(1) - ab_prev) / (F(1) - ab)) * np.sqrt(ops.one_minus_ratio(ab, ab_prev))
            mean_pred = x0 * np.sqrt(ab_prev) + ops.direction(ab_prev, sigma) * eps
            term = mask * sigma * z
            sample = mean_pred + term                                 # :584
    out = {"sample": sample, "pred_xstart": x0, "mean": mean, "log_variance": logvar, "noise_term": term}
    return {k: np.array(a, dtype=F, order="C") for k, a in out.items()}        # copies: no output aliases an input


# ------------------------------------------------------------------------------------------------------- comparator
def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def compare(got, ref, bound=None):
    """Element by element, nothing excluded.  The NaN pattern must be the reference's; every other element is
    bit-equal where `bound` is None or the reference is infinite, else within bound[element] (float64).
    -> the number of elements that fail."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == F
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    bad = nan_g != nan_r
    live = ~nan_g & ~nan_r
    equal = _bits(got) == _bits(ref)
    if bound is None:
        bad |= live & ~equal
    else:
        with np.errstate(all="ignore"):
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            within = np.where(np.isfinite(ref), err <= bound, equal)
        bad |= live & ~within
    return int(bad.sum())


def check(kind, got_sample, got_x0, ref, t):
    """The bars of the step tests, per element, with u = 2^-24.
    pred_xstart, every DDIM sample and the DDPM sample of a row at t == 0: bit-equal (add, multiply, divide and sqrtf
    are IEEE operations on the device; contraction is off).
    DDPM sample of a row at t > 0: |got - ref| <= 4u |sigma z| + 2u |ref|.  The device expf is within 1 ulp of the
    true value and the reference's is correctly rounded, so the two fp32 values of sigma are at most 1 ulp <= 2u
    sigma apart; the product with z rounds once on each side (2u + u + u = 4u of the term), and the final sum rounds
    once on each side (2u of the result).
    -> {name: failing elements}, empty when everything passes."""
    fails = {}
    n = compare(got_x0, ref["pred_xstart"])
    if n:
        fails["pred_xstart"] = n
    bound = None
    if kind == "ddpm":
        with np.errstate(all="ignore"):
            bound = 4 * U * np.abs(ref["noise_term"].astype(np.float64)) + 2 * U * np.abs(ref["sample"].astype(np.float64))
        bound[np.asarray(t) == 0] = 0.0
        exact = compare(got_sample[np.asarray(t) == 0], ref["sample"][np.asarray(t) == 0])
        if exact:
            fails["sample at t == 0"] = exact
    n = compare(got_sample, ref["sample"], bound)
    if n:
        fails["sample"] = n
    return fails


# ----------------------------------------------------------------------------------------------------------- inputs
def inputs(respacing, N, voxels, t, learn_sigma, predict_xstart, seed):
    """(mo, x, z) for one launch, from a seeded numpy generator.  x is the forward process at t of a unit-variance
    x_start and a unit normal eps, and the model output's first half is that eps (or that x_start under
    predict_xstart): at every t the x0 the step derives is the unit-variance x_start again, give or take the
    rounding of its large cancelling products, so about 32 % of it lies outside the clip's [-1, 1] whatever t is.
    The second half (the variance fraction) is uniform on [-1.2, 1.2]."""
    rng = np.random.default_rng(seed)
    tb = schedule(respacing)
    xs, eps, z = (rng.standard_normal((N, voxels)) for _ in range(3))
    t = np.asarray(t, dtype=np.int64)
    x = tb["sqrt_alphas_cumprod"][t][:, None] * xs + tb["sqrt_one_minus_alphas_cumprod"][t][:, None] * eps
    halves = [xs if predict_xstart else eps]
    if learn_sigma:
        halves.append(rng.uniform(-1.2, 1.2, (N, voxels)))
    mo = np.stack(halves, axis=1)
    return tuple(np.ascontiguousarray(a, dtype=F) for a in (mo, x, z))


def outside_share(x0_unclipped):
    """share of the finite unclipped x0 values outside [-1, 1]: the tests hold it between 10 % and 60 %"""
    a = x0_unclipped[np.isfinite(x0_unclipped)]
    return float((np.abs(a) > 1).mean())


def scatter(a, seed, per_kind=3):
    """NaN, +Inf and -Inf, `per_kind` of each, at seeded distinct positions of every row of a's last axis (all of
    them where the row is shorter than that) -> a poisoned copy"""
    a = a.copy()
    rng = np.random.default_rng(seed)
    flat = a.reshape(-1, a.shape[-1])
    values = [F("nan"), F("inf"), F("-inf")]
    for row in flat:
        pos = rng.permutation(row.size)[:3 * per_kind]
        for k, p in enumerate(pos):
            row[p] = values[k % 3]
    return a


# ------------------------------------------------------------------------------------------------------------ cases
FLAGS = [(learn, px, clip) for learn in (True, False) for px in (False, True) for clip in (True, False)]
T10 = ([9, 0, 4], [0, 9, 1])                       # the masked step among unmasked ones, in both positions
T1000 = ([999, 0, 1], [1, 500, 0])


def _case(name, kind, **kw):
    c = dict(name=name, kind=kind, respacing="10", ts=T10, voxels=257, learn=True, px=False, clip=True,
             etas=(0.0,) if kind == "ddpm" else (0.7,), sigma_small=False, variant="plain", poison=())
    c.update(kw)
    return c


def _cases():
    out = []
    for kind in ("ddpm", "ddim"):
        etas = (0.0,) if kind == "ddpm" else (0.0, 0.7, 1.0)
        # kind x flags, mixed t, 257 voxels (a second workgroup holding one voxel)
        for learn, px, clip in FLAGS:
            out.append(_case("%s-flags-%d%d%d" % (kind, learn, px, clip), kind, learn=learn, px=px, clip=clip,
                             etas=etas))
        # the unspaced schedule, where 1 - ab / ab_prev cancels to 1e-4
        for learn, px in ((True, False), (False, False), (True, True)):
            out.append(_case("%s-t1000-%d%d" % (kind, learn, px), kind, respacing="", ts=T1000, learn=learn, px=px,
                             etas=etas))
        # the fixed small variance
        out.append(_case("%s-sigma-small" % kind, kind, learn=False, sigma_small=True))
        out.append(_case("%s-sigma-small-t1000" % kind, kind, respacing="", ts=T1000, learn=False, sigma_small=True))
        # sizes: one voxel, a ragged single workgroup, and a second grid pass with a ragged tail at N = 2
        for voxels in (1, 255):
            out.append(_case("%s-voxels-%d" % (kind, voxels), kind, voxels=voxels))
        out.append(_case("%s-voxels-%d" % (kind, STRIDE + 257), kind, voxels=STRIDE + 257, ts=([9, 0], [0, 9])))
        # the _x0 entries: a finished x0; the parts of the model output their contract leaves unread hold NaN
        for clip in (True, False):
            for learn in ((True, False) if kind == "ddpm" else (True,)):
                out.append(_case("%s-x0-%d%d" % (kind, learn, clip), kind, variant="x0", learn=learn, clip=clip))
        # NaN, +Inf, -Inf scattered into the model output (both halves) and, separately, into x
        for clip in (True, False):
            out.append(_case("%s-nonfinite-%d" % (kind, clip), kind, clip=clip, poison=("mo", "x")))
    return out


CASES = _cases()


def launches(case):
    """Every launch of a case: (label, kwargs of step()).  The same arrays reach the kernel and the restatement."""
    seed = 1000 + [c["name"] for c in CASES].index(case["name"])
    for ti, t in enumerate(case["ts"]):
        N = len(t)
        mo, x, z = inputs(case["respacing"], N, case["voxels"], t, case["learn"], case["px"], seed + 100 * ti)
        xstart = None
        if case["variant"] == "x0":
            xstart = np.random.default_rng(seed + 7).standard_normal(x.shape).astype(F)
            mo = mo.copy()
            if case["kind"] == "ddpm" and case["learn"]:
                mo[:, 0] = np.nan                         # only the variance half is read
            else:
                mo[:] = np.nan                            # nothing of it is read
        variants = [("", mo, x)]
        if case["poison"]:
            variants = [("-" + p, scatter(mo, seed + 1) if p == "mo" else mo, scatter(x, seed + 2) if p == "x" else x)
                        for p in case["poison"]]
        for tag, mo_, x_ in variants:
            for eta in case["etas"]:
                yield ("%s-t%d%s-eta%g" % (case["name"], ti, tag, eta),
                       dict(kind=case["kind"], respacing=case["respacing"], mo=mo_, x=x_, z=z, t=list(t),
                            learn_sigma=case["learn"], predict_xstart=case["px"], clip=case["clip"], eta=eta,
                            xstart=xstart, sigma_small=case["sigma_small"]))


def share_of(kw):
    """outside_share of a launch's unclipped x0 (its xstart for the _x0 entries)"""
    if kw["xstart"] is not None:
        return outside_share(kw["xstart"])
    return outside_share(step(**dict(kw, clip=False))["pred_xstart"])


# ------------------------------------------------------------------------- the other users of the kernel's x0 helper
def reverse_step(respacing, mo, x, t, clip):
    """ddim_reverse_sample (:587-623) under eps-prediction, one fp32 rounding at a time -> sample, pred_xstart"""
    tb = schedule(respacing)
    t = np.asarray(t, dtype=np.int64)

    def c(table):
        return np.asarray(table, dtype=np.float64)[t].astype(F)[:, None]

    with np.errstate(all="ignore"):
        c_recip, c_recipm1 = c(tb["sqrt_recip_alphas_cumprod"]), c(tb["sqrt_recipm1_alphas_cumprod"])
        x0 = c_recip * x - c_recipm1 * mo[:, 0]
        if clip:
            x0 = np.clip(x0, F(-1), F(1))
        eps = (c_recip * x - x0) / c_recipm1                          # :611-614
        ab_next = c(tb["alphas_cumprod_next"])
        sample = x0 * np.sqrt(ab_next) + np.sqrt(F(1) - ab_next) * eps   # :615-621
    return {"sample": sample.astype(F), "pred_xstart": x0.astype(F)}
