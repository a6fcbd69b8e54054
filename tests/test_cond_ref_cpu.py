"""
tests/cond_ref.py without a GPU: the restatement of the conditioning path against oracle/unet_ref, against the
reference's recorded embeddings (tests/golden/timestep_embedding.npz) and against the reference's recorded run of the
whole path (tests/golden/cond.npz); the embedding evaluated a second way, with long-double cos / sin, on exactly the GPU
test's inputs, disagreeing on no more elements than the GPU test's cap; and the GPU tests' comparator against every
mutant of cond_ref.MUTANTS on every case of the mutant's stage, which it has to see at ten times the case's bar
(cond_ref.IDENTITY names the cases a mutant cannot change -- there its result must be bit-identical -- and cond_ref's
SiLU-probe comment the one mutant that arithmetic keeps below ten times any honest bar).
"""

import functools

import numpy as np
import pytest
import torch

import cond_ref as CR
from guided_diffusion import script_util as su
from guided_diffusion import synth
from oracle import unet_ref

F = np.float32
ORACLE_ATOL = 2e-7


# ----------------------------------------------------------------------------------------------------- embedding
def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / CR.ulp_bar(b)


def test_embedding_against_the_oracle_and_the_recorded_reference(golden):
    """The reference's recorded embeddings (tests/golden/timestep_embedding.npz, one machine's torch, the same file
    everywhere): bit-equal wherever that torch's fp32 cos / sin returned the correctly rounded value, within one ulp
    elsewhere.  oracle/unet_ref on this host's torch: the same on hosts whose vectorised fp32 cos / sin keep one ulp of
    the result; not every host's do -- next to a zero crossing, where the result is small, some keep an absolute
    error instead -- so an element off by more than an ulp is held to ORACLE_ATOL, the absolute bar
    tests/test_gpu_ops.py::test_linear_and_timestep_embedding already holds the kernel to against this oracle.  The
    split is printed."""
    g = golden("timestep_embedding.npz")
    equal = off = 0
    for d in (128, 32, 33):
        mine, theirs = CR.timestep_embedding(g["t"].astype(F), d, CR.freq_table(d)), g["e%d" % d]
        assert mine.shape == theirs.shape and theirs.dtype == F
        u = _ulps(theirs, mine)
        # the recorded table is the recording host's torch.exp, an ulp from this host's at the most: the argument
        # moves by t ulp(f) and by the rounding of the product, the result by no more (|sin|, |cos| <= 1)
        f, t = CR.freq_table(d), g["t"].astype(F)
        moved = t.astype(np.float64)[:, None] * np.spacing(f).astype(np.float64)[None]
        moved = moved + np.spacing(t[:, None] * f[None]).astype(np.float64) * (moved > 0)
        moved = np.concatenate([moved, moved] + ([np.zeros((len(t), 1))] if d % 2 else []), axis=1)
        same_table = u.max() <= 1.0
        assert (np.abs(theirs.astype(np.float64) - mine) <= CR.ulp_bar(mine) + (0 if same_table else 1) * moved).all(), d
        equal += int((u == 0).sum())
        off += int((u != 0).sum())
    print("embedding vs the recorded reference: %d elements bit-equal, %d not (one ulp where this host's frequency "
          "table is the recording host's: %s)" % (equal, off, same_table))
    assert equal > 0.5 * (equal + off)
    pad = CR.timestep_embedding(g["t"].astype(F), 33, CR.freq_table(33))[:, -1]
    assert np.array_equal(pad.view(np.uint32), np.zeros(4, np.uint32))
    equal = off = far = 0
    worst = 0.0
    for case in CR.EMB_CASES:
        t = CR.emb_times(case["kind"])
        mine = CR.timestep_embedding(t, case["dim"], CR.freq_table(case["dim"]))
        theirs = unet_ref.timestep_embedding(torch.from_numpy(t), case["dim"]).numpy()
        assert mine.shape == theirs.shape and theirs.dtype == F
        u = _ulps(theirs, mine)
        d = np.abs(theirs.astype(np.float64) - mine.astype(np.float64))
        assert (d[u > 1.0] <= ORACLE_ATOL).all(), (case["name"], d[u > 1.0].max())
        equal += int((u == 0).sum())
        off += int(((u != 0) & (u <= 1.0)).sum())
        far += int((u > 1.0).sum())
        worst = max(worst, float(d[u > 1.0].max()) if (u > 1.0).any() else 0.0)
    print("embedding vs the oracle on this host's torch: %d elements bit-equal, %d one ulp off, %d further off "
          "(largest of those %.3g absolute)" % (equal, off, far, worst))
    assert equal > 0.5 * (equal + off + far)


def test_embedding_reference_evaluated_two_ways_stays_within_the_cap():
    """fp64 and long-double cos / sin of the same fp32 argument, each rounded once to fp32, on the GPU test's inputs:
    the elements on which they differ are the ones a correctly working kernel may differ on as well."""
    if np.finfo(np.longdouble).nmant <= 52:
        pytest.skip("long double is double on this host")
    flips = total = 0
    for case in CR.EMB_CASES:
        t, dim = CR.emb_times(case["kind"]), case["dim"]
        a = CR.timestep_embedding(t, dim, CR.freq_table(dim))
        b = CR.timestep_embedding(t, dim, CR.freq_table(dim), longdouble=True)
        assert _ulps(a, b).max() <= 1.0
        flips += int((a.view(np.uint32) != b.view(np.uint32)).sum())
        total += a.size
    print("embedding fp64 vs long double: %d of %d elements differ" % (flips, total))
    assert flips <= CR.EMB_FLIP_CAP


# ------------------------------------------------------------------------------------------------------- the path
@functools.lru_cache(maxsize=None)
def model(tag):
    """(parameters the path reads, topology, film flag) of cond_ref.MODELS[tag], no weights allocated"""
    over, seed = CR.MODELS[tag]
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(over)
    with torch.device("meta"):
        m, _ = su.sr_create_model_and_diffusion(**fl)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    return CR.cond_params(shapes, seed, synth.synth_param), m.topology, m.use_scale_shift_norm


def sched_times(tag):
    steps, resp, rescale = CR.SCHEDULES[tag]
    d = su.create_gaussian_diffusion(steps=steps, learn_sigma=True, timestep_respacing=resp, rescale_timesteps=rescale)
    return d._model_timesteps(torch.arange(d.num_timesteps)).to(torch.float32).numpy()


def test_schedules_are_what_the_cases_say():
    assert len(sched_times("250")) == 250 and len(sched_times("10")) == 10
    assert sched_times("250").max() == 999 and sched_times("250").min() == 0
    assert np.array_equal(sched_times("250"), sched_times("250_rescaled"))      # 1000 / 1000: the same numbers
    assert {0.0, 999.0} <= set(CR.GOLDEN_T.tolist()) and (CR.GOLDEN_T % 1 != 0).sum() >= 4


@pytest.mark.parametrize("tag", list(CR.MODELS))
def test_film_rows_against_the_recorded_reference(golden, tag):
    """|fp64 restatement - the reference's fp32 run| within the bound of an fp32 run of unknown summation order."""
    g = golden("cond.npz")
    params, topo, film = model(tag)
    R = CR.GOLDEN_ROWS[tag]
    assert np.array_equal(g["t"], CR.GOLDEN_T) and g[tag + "/rows"].shape[0] == R
    y = None
    if "label_emb.weight" in params:
        y = CR.golden_labels(R, params["label_emb.weight"].shape[0])
        assert np.array_equal(g[tag + "/y"], y)
    # the recorded rows are emb_layers' output: the additive variant's conv-bias fold is the engine's, not the reference's
    ref = CR.film_rows(params, topo, CR.GOLDEN_T[:R], y, film, arith="torch", mut=None if film else "film_no_conv_bias_fold")
    assert ref["rows"].shape == g[tag + "/rows"].shape
    e_emb = CR.excess(g[tag + "/emb"], ref["e2"], ref["bound_e2"])
    e_rows = CR.excess(g[tag + "/rows"], ref["rows"], ref["bound"])
    print("%s: recorded reference vs fp64, |diff| / bound: emb %.3f, rows %.3f" % (tag, e_emb, e_rows))
    assert e_emb <= 1.0 and e_rows <= 1.0
    # the kernels' own bound is the tighter of the two (their chains are 64 times shorter)
    own = CR.film_rows(params, topo, CR.GOLDEN_T[:R], y, film)
    assert (own["bound"] <= ref["bound"]).all()


# -------------------------------------------------------------------------------------------------------- mutants
MARGIN = 10.0


def _judge(name, case, clean, mutant, bar, seen, margin=MARGIN):
    """clean / mutant: what the kernel would leave in its output buffer"""
    assert CR.excess(clean, clean, bar) == 0.0
    same = CR.bits_equal(np.nan_to_num(clean, nan=-7.0), np.nan_to_num(mutant, nan=-7.0))
    ident = CR.IDENTITY.get(name, lambda c: False)(case)
    assert same == ident, (name, case["name"], "identical" if same else "differs")
    if not same:
        e = CR.excess(mutant, clean, bar)
        assert e >= margin, (name, case["name"], e)
        seen.append(e)


def _mutants(stage):
    names = [k for k, v in CR.MUTANTS.items() if v == stage]
    assert names
    return names


def test_cases_cover_the_axes():
    assert {c["dim"] for c in CR.EMB_CASES} == {2, 6, 32, 128, 129, 512}
    assert {len(CR.emb_times(c["kind"])) for c in CR.EMB_CASES} == {1, 5, 1000}
    sizes = {len(CR.emb_times(c["kind"])) * c["dim"] % 256 == 0 for c in CR.EMB_CASES}
    assert sizes == {True, False}
    assert {c["K"] for c in CR.LIN_CASES} == {1, 63, 64, 65, 100, 128, 512}
    assert {c["O"] for c in CR.LIN_CASES} == {1, 3, 4, 5, 70, 514}
    assert {c["rows"] for c in CR.LIN_CASES} == {1, 7, 8, 9, 17, 1000}
    shapes = set(CR.LIN_SHAPES)
    for r in (7, 8, 9):                       # each neighbour of 8 rows meets each neighbour of 64 columns ...
        assert {K for rr, K, O in shapes if rr == r} >= {63, 64, 65}
    for K in (63, 64, 65):                    # ... and each of those each neighbour of 4 outputs
        assert {O for rr, KK, O in shapes if KK == K} >= {3, 4, 5}
    assert len(shapes) == len(CR.LIN_SHAPES) and 18 <= len(shapes) <= 24
    assert {(c["rows"], c["dim"], c["nc"]) for c in CR.LAB_CASES} == {(r, d, n) for r in (1, 5, 300)
                                                                     for d in (1, 7, 512) for n in (1, 10)}
    assert len(CR.MUTANTS) == 15


def test_embedding_mutants_are_seen():
    seen = []
    for case in CR.EMB_CASES:
        t, dim = CR.emb_times(case["kind"]), case["dim"]
        clean = CR.timestep_embedding(t, dim, CR.freq_table(dim))
        for name in _mutants("emb"):
            _judge(name, case, clean, CR.timestep_embedding(t, dim, CR.freq_table(dim), mut=name), CR.ulp_bar(clean),
                   seen)
    print("embedding mutants: smallest excess %.3g ulp" % min(seen))


def test_linear_mutants_are_seen():
    seen = []
    for case in CR.LIN_CASES:
        x, w, b, small = CR.lin_inputs(case)
        val, _ = CR.linear(x, w, b, case["silu"])
        bar = CR.linear_bar(x, w, b, case["silu"])
        # the small column is small: a norm over the whole output could not hold it to anything
        if case["O"] > 1:
            assert np.abs(val[:, small]).max() < 1e-3 * np.abs(np.delete(val, small, axis=1)).max()
        assert (bar <= 21 * CR.U * (np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
                                    + np.abs(b.astype(np.float64)))).all()
        for name in _mutants("lin"):
            mv, _ = CR.linear(x, w, b, case["silu"], mut=name)
            _judge(name, case, CR.place(val, case["O"]), CR.place(mv, case["O"]), bar, seen)
        gap = case["O"] + CR.GAP
        bar_gap = np.concatenate([bar, np.ones((case["rows"], CR.GAP))], axis=1)
        for name in _mutants("lin_strided"):
            _judge(name, case, CR.place(val, gap), CR.place(val, gap, mut=name), bar_gap, seen)
    print("linear mutants: smallest excess %.3g bars" % min(seen))


def test_fast_math_silu_is_seen_by_the_probe():
    """cond_ref's SiLU-probe comment: this mutant exceeds the 5u bar, and cannot exceed ten times it."""
    clean, bar = CR.silu_probe_ref()
    mutant, _ = CR.silu_probe_ref("lin_fast_silu")
    e = CR.excess(mutant, clean, bar)
    print("fast-math SiLU on the probe: %.3f bars" % e)
    assert 1.5 <= e <= 8.0 / 5.0 + 1e-3
    # and, as computed there, it stays below the per-element bar of every linear case
    for case in CR.LIN_CASES:
        if case["silu"]:
            x, w, b, _ = CR.lin_inputs(case)
            assert CR.excess(CR.linear(x, w, b, 1, "lin_fast_silu")[0], CR.linear(x, w, b, 1)[0],
                             CR.linear_bar(x, w, b, 1)) < 1.0


def test_label_mutants_are_seen():
    seen = []
    for case in CR.LAB_CASES:
        launches = CR.lab_launches(case)
        for name in _mutants("lab"):
            clean = np.concatenate([CR.add_embedding(*l) for l in launches])
            mutant = np.concatenate([CR.add_embedding(*l, mut=name) for l in launches])
            _judge(name, case, clean, mutant, CR.ulp_bar(clean), seen)
        ys = np.concatenate([l[2] for l in launches])
        assert {0, case["nc"] - 1, -1, case["nc"], 2 ** 40} <= set(ys.tolist())
    print("label mutants: smallest excess %.3g ulp" % min(seen))


@pytest.mark.parametrize("tag", list(CR.MODELS))
def test_film_mutants_are_seen(tag):
    """Against the end-to-end bound, on every schedule of the GPU test and on the golden's timesteps."""
    params, topo, film = model(tag)
    seen = []
    times = {s: sched_times(s) for s in CR.SCHEDULES}
    times["golden"] = CR.GOLDEN_T[:CR.GOLDEN_ROWS[tag]]
    for s, t in times.items():
        case = dict(name="%s_%s" % (tag, s), film=film)
        y = CR.golden_labels(len(t), params["label_emb.weight"].shape[0]) if "label_emb.weight" in params else None
        clean = CR.film_rows(params, topo, t, y, film)
        names = _mutants("film") + (["lab_row_off_by_one"] if y is not None else [])
        for name in names:
            mutant = CR.film_rows(params, topo, t, y, film, mut=name)
            _judge(name, case, clean["rows"].astype(F), mutant["rows"].astype(F), clean["bound"], seen)
        if y is not None:                     # dropping the label add altogether
            _judge("no_label", case, clean["rows"].astype(F), CR.film_rows(params, topo, t, None, film)["rows"].astype(F),
                   clean["bound"], seen)
    print("%s film mutants: smallest excess %.3g bounds" % (tag, min(seen)))
