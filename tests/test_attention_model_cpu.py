"""
The attention reference, cases and f16x3 model (attention_ref.py) on the CPU tier: the reference against the
oracle's, the un-mutated model against the reference on every case of test_gpu_attention.py (within a tenth of
the bars the kernel is held to), that every plausible kernel bug moves some case by at least 10x its bar, and
the facts about loose and understated bounds that the GPU cases rest on.
"""

import numpy as np
import pytest
import torch

import attention_ref as R

TENTH = 0.1


def _model(c, mut=()):
    return R.model(c.qkv, c.heads, c.ch, c.bound, c.offset, c.count, c.stride, mut=mut)


_BASE = {}


def _base(name):
    """the un-mutated model's output of a case, computed once"""
    if name not in _BASE:
        _BASE[name] = _model(R.case(name))
    return _BASE[name]


def test_reference_is_the_oracles():
    """reference() on the kernel's channels-last layout = oracle/unet_ref.qkv_attention in fp64 on the reference's
    (N * heads, ch, T) layout, to 1e-12; ragged T, three heads, blocked and unblocked"""
    from oracle import unet_ref
    for N, T, heads, ch, block in [(2, 77, 3, 32, None), (1, 130, 2, 64, 48)]:
        g = np.random.default_rng(T)
        ref_layout = torch.from_numpy(g.standard_normal((N, heads * 3 * ch, T)).astype(np.float32))
        q, k, v = ref_layout.reshape(N * heads, ch * 3, T).split(ch, dim=1)
        want = unet_ref.qkv_attention(q, k, v, block=block, dtype=torch.float64).reshape(N, heads * ch, T)
        got = R.reference(ref_layout.permute(0, 2, 1).contiguous().numpy(), heads, ch)
        err = np.abs(got - want.permute(0, 2, 1).numpy()).max()
        assert err <= 1e-12 * float(want.abs().max()), err


def test_case_lists_are_complete():
    """every case belongs to one group, every group meets every head width, and the builders' guarantees hold
    (each builder asserts its own)"""
    assert set(R.GROUP.values()) == {"a", "b", "c"}
    for group in "abc":
        assert {R.case(n).ch for n in R.names(group)} == {32, 64, 128}, group
    for n in R.CASES:
        c = R.case(n)
        assert c.qkv.dtype == np.float32 and c.bound.dtype == np.float32
        assert c.T <= 300 and c.N <= 3 and c.heads <= 2
        assert c.offset + ((c.N * c.count - 1) * c.stride) < c.bound.size      # every entry inside the allocation


@pytest.mark.parametrize("name", R.CASES)
def test_model_is_within_a_tenth_of_the_bars(name):
    """The un-mutated model of the f16x3 arithmetic against the fp64 reference, per case: within a tenth of the
    per (sample, head) bar (1e-5) and of the per query row bar (1e-4) -- measured 0.6e-7 .. 3.8e-7 per head and at
    most 9.0e-7 per row; within the stated element bound on the one-hot cases (0.20 of it), exactly 0 on the
    all-zero case, non-finite everywhere on the understated bound."""
    c, got, ref = R.case(name), _base(name), R.case_reference(name)
    if c.kind == "zero":
        assert (got == 0).all()
    elif c.kind == "loud":
        ok = np.abs(got - ref) <= R.BAR * np.abs(ref).max()
        assert (~np.isfinite(got) | ok).all() and not np.isfinite(got).all()
        print("%s: %.3f of the outputs are finite" % (name, np.isfinite(got).mean()))
    else:
        assert np.isfinite(got).all()
        if c.kind == "onehot":
            sel, bound = R.one_hot_expected(c)
            worst = float((np.abs(got - sel) / bound).max())
            print("%s: %.3g of the element bound" % (name, worst))
            assert worst <= 1.0
        per_head, per_row = R.head_errors(got, ref, c.heads, c.ch)
        print("%s: per (sample, head) %.3g, per row %.3g" % (name, per_head.max(), per_row.max()))
        assert per_head.max() < TENTH * R.BAR and per_row.max() < TENTH * R.ROW_BAR


# mutation -> the cases that are there for it (measured ratio of each in the docstring below)
CASES_FOR = {
    "sample0_scale": ["samples_1_tiny", "samples_tiny_1", "samples_1_tiny_small"],
    "first_entry_only": ["entries32_max_last", "entries33_max_last", "entries64_max_last"],
    "ignore_stride": ["wiring_like", "entries32_max_last", "entries32_max_first", "entries1", "entries33_max_last"],
    "ignore_offset": ["wiring_like", "entries32_max_last", "entries32_max_first", "entries1", "entries33_max_last"],
    "no_mask": ["all_negative_T77", "all_negative_T45", "all_negative_T77_ch64", "edge_T1", "edge_T33"],
    "no_rescale": ["rising_T160", "rising_T300", "mixed_even_rising", "mixed_odd_rising", "one_hot_T109"],
    "no_l_rescale": ["rising_T160", "rising_T300", "mixed_even_rising", "mixed_odd_rising", "one_hot_T77"],
    "rescale_by_first_query": ["mixed_odd_rising", "one_hot_T109", "one_hot_T77", "one_hot_T45"],
    "drop_q_lo": ["loose_x1", "loose_x40", "loose_x4096", "edge_T127"],
    "drop_k_lo": ["loose_x1", "loose_x40", "loose_x4096", "edge_T129"],
    "drop_v_lo": ["loose_x1", "edge_T1", "uniform_T100", "one_hot_T109"],
    "drop_p_lo": ["loose_x1", "loose_x40", "rising_T160", "edge_T257"],
    "scale_once": ["rising_T160", "falling_T160", "tail_max_T77", "edge_T2"],
}


def test_every_bug_has_a_case():
    assert set(CASES_FOR) == set(R.MUTATIONS) and len(CASES_FOR) == 13
    assert all(n in R.CASES for names in CASES_FOR.values() for n in names)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_bugs_move_the_output_beyond_the_bar(mut):
    """Discrimination: each mutation of the model moves the output of each of its cases by at least 10x the
    per (sample, head) bar at some (sample, head); a non-finite output counts as moved (inf).  Measured ratios
    (moved / 1e-5):

      sample0_scale           samples_1_tiny 44, samples_tiny_1 inf, samples_1_tiny_small 64.  (With the samples
                              a thousand-fold apart and 33x-loose bounds, wiring_like moves by 0.02: only a gap
                              well over 2^20 shows a wrong sample's scale.)
      first_entry_only        entries32 / 33 / 64 _max_last: inf (the 2^-30 entry overflows f16)
      ignore_stride, ignore_offset
                              wiring_like, entries32_*, entries1, entries33_max_last: 1e5 each (the 1e30 column
                              underflows every operand to 0)
      no_mask                 all_negative_*: 1e5 (the padded keys take 0.9999 of the weight); edge_T1 9.9e4,
                              edge_T33 3.8e4
      no_rescale              rising_T160 2.9e5, rising_T300 3.5e5, mixed_even 3.0e5, mixed_odd 2.3e5,
                              one_hot_T109 6.4e5
      no_l_rescale            rising_T160 7.9e4, rising_T300 9.0e4, mixed_even 8.6e4, mixed_odd 8.5e4,
                              one_hot_T77 9.7e4
      rescale_by_first_query  mixed_odd_rising 2.3e5 (each wave's first query falls, so the rising queries are
                              never rescaled), one_hot_* 5.5e5 .. 7.0e5.  mixed_even_rising: 0 -- there the
                              first query rises and the decision happens to be right; that case is for the
                              ballot's other direction (a skipped rescale that a falling query's alpha == 1
                              would suggest).
      drop_q_lo               loose_x1 39, loose_x40 38, loose_x4096 31, edge_T127 48
      drop_k_lo               loose_x1 33, loose_x40 32, loose_x4096 40, edge_T129 29
      drop_v_lo               loose_x1 30, edge_T1 47, uniform_T100 28, one_hot_T109 44
      drop_p_lo               loose_x1 19, loose_x40 23, rising_T160 38, edge_T257 14
      scale_once              rising_T160 7.2e4, falling_T160 1.3e5, tail_max_T77 1.7e3, edge_T2 3.8e4
    """
    for name in CASES_FOR[mut]:
        c, base = R.case(name), _base(name)
        moved, _ = R.head_errors(_model(c, mut), base, c.heads, c.ch)
        ratio = float(moved.max() / R.BAR)
        print("%s / %s: %.3g" % (mut, name, ratio))
        assert ratio >= 10.0, (mut, name, ratio)


def test_bound_looseness_and_understatement():
    """What the bound cases rest on, on Gaussian data whose maximum is 1.5 x 2^k: a bound up to 2^12 loose is free
    (within a tenth of the bar: measured 1.1e-7 at 1x and 40x, 1.3e-7 at 2^12), 2^24 loose is beyond the bar (2.9e-4),
    half the true bound still gives finite results within a tenth of the bar (the scaled maximum 1.5 x 2^15 is
    below f16's 65504), and a quarter gives no finite output at all."""
    g = np.random.default_rng(5).standard_normal((1, 96, 2 * 3 * 64))
    qkv = (g * (3.0 / np.abs(g).max())).astype(np.float32)
    assert np.abs(qkv).max() == np.float32(3.0)
    ref = R.reference(qkv, 2, 64)

    def run(factor):
        out = R.model(qkv, 2, 64, np.array([3.0 * factor], np.float32), 0, 1, 1)
        return out, float(R.head_errors(out, ref, 2, 64)[0].max())

    for f in (1.0, 40.0, 2.0 ** 12):
        out, err = run(f)
        print("bound x %g: %.3g" % (f, err))
        assert err < TENTH * R.BAR
    out, err = run(2.0 ** 24)
    print("bound x 2^24: %.3g" % err)
    assert np.isfinite(out).all() and err > R.BAR
    out, err = run(0.5)
    print("bound x 1/2: %.3g" % err)
    assert np.isfinite(out).all() and err < TENTH * R.BAR
    out, _ = run(0.25)
    assert not np.isfinite(out).any()


def test_scale_rule():
    """qkv_scale's rule at its edges: the exponent of a power of two and of the float below it, the clamp to
    2^+-40, S = 1 for 0, a negative bound, inf and NaN, a NaN entry dropped by the max, the entries of sample n at
    (n * count + i) * stride"""
    assert R.scale_exponent(4.0) == 12 and R.scale_exponent(np.nextafter(np.float32(4.0), np.float32(0))) == 13
    assert R.scale_exponent(1.0) == 14 and R.scale_exponent(2.0 ** 15) == -1
    assert R.scale_exponent(1e-30) == 40 and R.scale_exponent(1e30) == -40 and R.scale_exponent(1e-45) == 40
    for b in (0.0, -3.0, np.inf, np.nan):
        assert R.scale_exponent(b) == 0
    arr = np.array([9e9, 1.0, 9e9, np.nan, 9e9, 0.5, 9e9, 16.0, 9e9, 2.0], np.float32)
    assert R.qkv_scale(arr, 1, 2, 2, 0) == 2.0 ** 14 and R.qkv_scale(arr, 1, 2, 2, 1) == 2.0 ** 10
    assert R.qkv_scale(arr, 1, 2, 2, 1, mut={"sample0_scale"}) == 2.0 ** 14
    assert R.qkv_scale(arr, 1, 2, 2, 1, mut={"first_entry_only"}) == 2.0 ** 15
    assert R.qkv_scale(arr, 1, 2, 2, 0, mut={"ignore_offset"}) == 2.0 ** -19
