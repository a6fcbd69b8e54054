"""
The GroupNorm reference (gn_ref.py) on the CPU tier: finalize_ref against torch's fp64 group_norm, per case of
test_gpu_groupnorm.py that each plausible kernel bug moves A, B or the bound by at least 10x the bar the GPU test
holds that case to, and the GnAcc emulation against its derived slack delta(n).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_ref as R
import test_gpu_groupnorm as G


@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("groups,C0,C1", [(32, 64, 0), (4, 24, 8), (1, 12, 0), (20, 20, 0)])
def test_finalize_ref_is_group_norm(film, groups, C0, C1):
    """A x + B  ==  group_norm(x) * (1 + scale) + shift in fp64, over a virtual concat with different, uneven row
    partitions per source (empty rows included)"""
    g = np.random.default_rng(groups + C0)
    N, V, C = 3, 75, C0 + C1
    xs = [(g.standard_normal((N, Ci, V)) * 3 + 1.5).astype(np.float32) for Ci in (C0, C1) if Ci]
    st = [R.make_stats(x, R.partition(g, V, rows, empty=0.3)) for x, rows in zip(xs, (9, 4))]
    gamma, beta = g.standard_normal(C).astype(np.float32), g.standard_normal(C).astype(np.float32)
    stride, off = 2 * C + 11, 5
    fm = g.standard_normal((N, stride)).astype(np.float32) if film else None
    r = R.finalize_ref(st[0], st[1] if C1 else None, V, 1e-5, gamma, beta, fm, stride, off, groups)
    x = torch.from_numpy(np.concatenate(xs, axis=1)).double()
    want = F.group_norm(x, groups, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(),
                        eps=float(np.float32(1e-5)))
    if film:
        f = torch.from_numpy(fm).double()
        want = want * (1 + f[:, off:off + C, None]) + f[:, off + C:off + 2 * C, None]
    got = x * torch.from_numpy(r["A"])[:, :, None] + torch.from_numpy(r["B"])[:, :, None]
    assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max())
    # the bound entries bound, on exact sums
    xg = x.numpy().reshape(N, groups, -1)
    assert (r["xmax"] >= np.abs(xg).max(axis=2) * (1 - 1e-12)).all()
    assert (r["bound0"] >= np.abs(got.numpy().reshape(N, groups, -1)).max(axis=2) * (1 - 1e-12)).all()


def test_make_stats_rows():
    x = np.arange(24, dtype=np.float32).reshape(1, 2, 12)
    st = R.make_stats(x, [0, 5, 0, 7, 0])
    assert st.shape == (1, 2, 5, 2) and (st[:, :, [0, 2, 4]] == 0).all()
    assert st[0, 1, 1, 0] == sum(range(12, 17)) and st[0, 1, 3, 1] == sum(v * v for v in range(17, 24))


def mutations(c):
    """the plausible bugs that can show on case c (test_bugs_move_the_outputs_beyond_the_bar's docstring)"""
    m = {}
    threads = R.launch_threads(c.C0, c.rows0, c.C1, c.rows1, c.groups)
    live = c.data != "zero"
    if c.C1 and c.rows0 != c.rows1 and live:
        m["rows0 used for the second source"] = dict(rows0_for_src1=True)
    if c.C1 and live:
        m["a group of source 1 read from source 0"] = dict(group_from_src0=True)
    if live and any(rows * c.cg % (threads * 8) for rows in (c.rows0, c.rows1) if rows):
        m["last partial load pass dropped"] = dict(drop_last_pass=True)
    if c.film and c.gamma:
        m["sample 0's FiLM row for every sample"] = dict(film_sample0=True)
        m["shift row read at C // 2"] = dict(shift_half=True)
        if c.film_off:
            m["film_off ignored"] = dict(film_off_ignored=True)
    if c.gamma and c.cg > 1 and live:
        m["count not multiplied by the group width"] = dict(count_no_cg=True)
    if c.gamma and c.data in ("gauss", "const", "zero", "nan"):
        m["eps left out"] = dict(no_eps=True)
    if c.bound and live:
        m["maximum over the sums"] = dict(max_over_sums=True)
    return m


def test_every_bug_has_a_case_and_every_case_a_bug():
    seen = {name for c in G.CASES for name in mutations(c)}
    assert len(seen) == 9, seen
    assert all(mutations(c) for c in G.CASES)


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_bugs_move_the_outputs_beyond_the_bar(name):
    """Discrimination: each mutation moves A or B by at least 10x its element's bar (gn_ref.finalize_bars), or a
    bound entry by at least 10x what the GPU test allows it (test_gpu_groupnorm.bound_bars), somewhere; a NaN or
    infinity where the reference is finite counts as moved.

    Where a bug applies: the two concat bugs to the cases with a second source (rows0 for rows1 only where they
    differ); the dropped pass wherever a source's run is not a whole number of passes of 8 x blockDim items;
    the three FiLM bugs to the FiLM cases (the offset only where it is not zero); the count without the group
    width to groups wider than one channel; the row maximum to every case that asks for the bound.  None of these
    shows on all-zero rows, whose sums are zero however they are read.  eps left out moves rstd by
    eps / (2 (var + eps)) of itself: 5e-6 at unit variance against bars of a few 2^-24 -- it applies to the cases
    of unit-scale variance and to the degenerate ones (where it gives infinity), not to the mean of 1e3 standard
    deviations, whose bar carries the variance's cancellation term."""
    t = G.inputs(name)
    c, ref = t["case"], t["ref"]
    bar0, bar1 = G.bound_bars(t)
    for what, kw in mutations(c).items():
        mu = R.finalize_ref(*t["args"], mut=R.Mut(**kw))
        ratio = 0.0
        pairs = [(mu["xmax"], ref["xmax"], bar1), (mu["bound0"], ref["bound0"], bar0)] if c.bound else []
        if c.gamma:
            pairs += [(mu["A"], ref["A"], t["barA"]), (mu["B"], ref["B"], t["barB"])]
        with np.errstate(all="ignore"):
            for got, want, bar in pairs:
                ok = np.isfinite(want) & np.isfinite(bar)
                r = np.where(np.isfinite(got[ok]), np.abs(got[ok] - want[ok]) / np.maximum(bar[ok], 1e-300), np.inf)
                ratio = max(ratio, float(r.max()))
        print("%s / %s: %.3g" % (name, what, ratio))
        assert ratio >= 10.0, (what, ratio)


def test_bars_are_fp32_grade():
    """the bars are not loose: a few fp32 roundings relative to max(|A|, |beta| + |mean A|) on Gaussian data"""
    for name in ("items_6_film", "items_2049", "cat_64_64", "groups_2"):
        t = G.inputs(name)
        A, B = np.abs(t["ref"]["A"]), np.abs(t["ref"]["B"])
        assert (t["barA"] <= 8 * R.U32 * A + 1e-40).all()
        scale = B + np.abs(np.repeat(t["ref"]["mean"], t["case"].cg, axis=1)) * A * (1 + 0.5 * t["case"].film)
        assert (t["barB"] <= 12 * R.U32 * scale + 1e-40).all()


# --------------------------------------------------------------------------- GnAcc
def test_gnacc_is_exact_on_small_integers():
    g = np.random.default_rng(1)
    x = g.integers(-50, 50, (200, 33)).astype(np.float32)
    s1, s2 = R.gnacc_sums(x)
    assert np.array_equal(s1, x.astype(np.float64).sum(axis=1))
    assert np.array_equal(s2, (x.astype(np.float64) ** 2).sum(axis=1))


def test_hot_voxel_shortfall_is_real_and_within_delta():
    """one lane, the hot value first (= the pivot), 2 to 128 values, a background of 1e-3 of it: sqrt(sum2) does
    fall below the hot value -- the slack is needed -- and never by more than delta(n)"""
    g = np.random.default_rng(2)
    worst = 0.0
    for n in list(range(2, 33)) + [48, 64, 96, 128]:
        L = 4000
        hot = (g.uniform(1.0, 2.0, L) * 10.0 ** g.integers(-3, 4, L) * g.choice([-1.0, 1.0], L)).astype(np.float32)
        x = (1e-3 * np.abs(hot)[:, None] * (1 + 0.25 * g.uniform(-1, 1, (L, n)))).astype(np.float32)
        x[:, 0] = hot
        _, s2 = R.gnacc_sums(x)
        assert (s2 >= 0).all()
        short = 1.0 - np.sqrt(s2) / np.abs(hot.astype(np.float64))
        worst = max(worst, float(short.max()))
        assert short.max() <= R.delta(n) - 3 * R.U32, (n, float(short.max()), R.delta(n))
    print("largest shortfall %.3g; delta(2) %.3g, delta(16) %.3g, delta(64) %.3g, delta(128) %.3g"
          % (worst, R.delta(2), R.delta(16), R.delta(64), R.delta(128)))
    assert worst > 1e-6          # beyond what test_gpu_range.py's Gaussian case allows: the contract is not "upper bound"
    # ... and the activation scale's headroom under f16's largest value takes it in, for any lane the kernels have
    assert all(R.headroom_ok(R.delta(n)) for n in (1, 2, 4, 16, 64, 128, 1024))
    assert R.delta(1) == 3 * R.U32 and all(R.delta(n) < R.delta(n + 1) for n in range(1, 200))


def test_delta_holds_on_adversarial_lanes():
    """other shapes of lane: hot value anywhere, mixed signs, two hot values of opposite sign, all-equal"""
    g = np.random.default_rng(3)
    for n in (2, 3, 16, 64):
        L = 3000
        x = (1e-3 * g.standard_normal((L, n))).astype(np.float32)
        pos = g.integers(0, n, L)
        x[np.arange(L), pos] = g.choice([-1.0, 1.0], L) * g.uniform(1, 2, L)
        x[: L // 3, 0] = -x[np.arange(L // 3), pos[: L // 3]]          # pivot = a hot value of the other sign
        x[-10:] = x[-10:, :1]                                            # all equal
        _, s2 = R.gnacc_sums(x)
        m = np.abs(x.astype(np.float64)).max(axis=1)
        assert (np.sqrt(np.maximum(s2, 0)) >= m * (1 - R.delta(n))).all() and (s2 >= 0).all()


@pytest.mark.parametrize("bug", ["cross", "count", "pivot0"])
def test_gnacc_bugs_break_what_the_writers_are_held_to(bug):
    """test_bound_through_every_statistics_writer holds a group's sum of squares to sum2_slack(n) of the fp64 sum
    and the bound to max|x| (1 - delta(n)): on its hot-voxel lanes (the pivot hot: every lane of a tile's first
    rows) a wrong conversion misses one of the two by 10x or more"""
    g = np.random.default_rng(4)
    for n in (4, 16, 64):
        for bg in G.BACKGROUNDS:
            x = (bg * g.uniform(0.75, 1.25, (500, n))).astype(np.float32)
            x[:, 0] = g.uniform(1, 2, 500) * g.choice([-1.0, 1.0], 500)
            x = (x * 10.0 ** g.integers(-3, 4, (500, 1))).astype(np.float32)
            _, s2 = R.gnacc_sums(x, bug=bug)
            xd = x.astype(np.float64)
            T, M = (xd * xd).sum(axis=1), np.abs(xd).max(axis=1)
            with np.errstate(invalid="ignore"):
                short = np.nan_to_num(1.0 - np.sqrt(s2) / M, nan=np.inf)      # (a negative sum2: no bound at all)
            assert max((np.abs(s2 - T) / T).min() / R.sum2_slack(n), short.min() / R.delta(n)) >= 10.0


@pytest.mark.parametrize("vox,mean", [(255, 0.0), (256, 1e4), (1000, 0.0)])
def test_gn_stats_bar_tells_fp32_sums_and_a_lost_voxel(vox, mean):
    """the bar test_gn_stats_against_fp64 holds ddpm3d_gn_stats to (voxels 2^-53 sum|terms|): sums accumulated in
    fp32, or a row that misses its last voxel, are 10x beyond it"""
    g = np.random.default_rng(vox)
    x = (g.standard_normal((8, vox)) + mean).astype(np.float32)
    xl = x.astype(np.longdouble)
    for terms in (xl, xl * xl):
        bar = (vox * R.U64 * np.abs(terms).sum(axis=1)).astype(np.float64)
        exact = terms.sum(axis=1)
        f32 = np.cumsum(terms.astype(np.float32), axis=1, dtype=np.float32)[:, -1]
        assert (np.abs(f32 - exact).astype(np.float64) / bar).max() >= 10.0
        assert (np.abs(terms[:, :-1].sum(axis=1) - exact).astype(np.float64) / bar).min() >= 10.0
