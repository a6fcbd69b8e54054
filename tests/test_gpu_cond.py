"""
The conditioning path on the GPU -- ddpm3d_timestep_embedding, ddpm3d_linear (plain and SiLU-in), ddpm3d_add_embedding
and UNetEngine.film_rows, which chains them into the FiLM rows (or, in the additive variant, the first convs' per-sample
bias) of every ResBlock -- element by element against tests/cond_ref.py, the fp64 restatement of the reference's
timestep_embedding / time_embed / label_emb / emb_layers.  Cases, inputs, bars and comparator are cond_ref's, where the
bars are derived and where tests/test_cond_ref_cpu.py shows that the comparator sees fifteen kinds of kernel error on
these inputs.  Every output buffer starts NaN-filled, so an element a kernel leaves unwritten shows.

Bars (cond_ref's docstring has the derivations; u = 2^-24), per element, nothing excluded:
  embedding   one fp32 ulp of the reference, and at most 2 elements of the 1.6 million not bit-equal; pad column +0.0
  linear      gamma_m (sum |s_k w_k| + |b|) [+ 5u sum |s_k w_k| with SiLU-in], m = ceil(K / 64) + 6 + 1; one output
              column has weights 1e-5 of the others'; out_stride = O + 3 leaves the gap NaN and the written bits as they
              were; a row of a T-row call is bit-equal to the one-row call; a NaN in row 9 stays in row 9
  SiLU        K = 1, w = 1, b = 0 returns the kernel's SiLU itself: 5u |silu(x)| on 648 arguments in [-80, 80]; the
              tails -100, -88, 88, 100, +-0 stay finite, -100 contributes no more than 2^-120 |w|, +100 gives 100 w
  labels      bit-equal to one fp32 add; labels -1, num_classes, 2^40 leave their rows bit-identical
  film_rows   (a) each stage against cond_ref applied to the GPU's own previous stage, within that stage's bar, the last
              Linear against a fused matrix cond_ref assembles itself from the state_dict; (b) end to end against the
              reference implementation's recorded run (tests/golden/cond.npz), within the propagated bound of the
              kernels plus that of an fp32 run of unknown summation order; (c) rows of the T-row table bit-equal to
              one-row calls.

Largest |got - ref| / bar on an MI355X (each test prints its own):
  embedding      0 of 1 622 854 elements not bit-equal, largest difference 0 ulp
  linear         0.167 over the 44 launches (rows 1000, K 65, O 5, no SiLU); the small column 0.153 at most
  SiLU probe     0.335 of 5u |silu(x)|
  film_rows (a)  embedding 0.000; time_embed.0 0.240 (tiny) and 0.123 (published); time_embed.2 0.099 and 0.032;
                 emb_layers 0.102 (tiny, additive) and 0.041 (published)
  film_rows (b)  against the recorded reference 0.0014 of the summed bounds at most (tiny, additive), 0.0001 published;
                 against fp64 0.0039 of the kernels' own propagated bound at most
The worst-case bounds are several times what the kernels need: roundings do not all fall the same way.  What the
mutants exceed them by is printed by tests/test_cond_ref_cpu.py.
"""

import functools

import numpy as np
import pytest
import torch

import cond_ref as CR
from guided_diffusion import _hip as H
from guided_diffusion import script_util as su
from guided_diffusion import synth

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 64                                    # NaN-filled floats behind every output: nothing may be written there


def np_(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).cuda()


def nan_buf(n):
    return torch.full((n + TAIL,), float("nan"), device="cuda")


def tail_untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all()) and buf.numel() == n + TAIL


# ------------------------------------------------------------------------------------------------------ embedding
def test_timestep_embedding_is_the_correctly_rounded_value():
    lib, flips, total, worst = H.load(), 0, 0, 0.0
    for case in CR.EMB_CASES:
        t, dim = CR.emb_times(case["kind"]), case["dim"]
        rows = len(t)
        freqs = CR.freq_table(dim)
        ref = CR.timestep_embedding(t, dim, freqs)
        td, fd, out = dev(t), dev(freqs), nan_buf(rows * dim)
        H.check(lib.ddpm3d_timestep_embedding(H.ptr(td), rows, dim, H.ptr(fd), H.ptr(out), H.stream()))
        got = np_(out[:rows * dim]).reshape(rows, dim)
        assert tail_untouched(out, rows * dim), case["name"]
        e = CR.excess(got, ref, CR.ulp_bar(ref))
        assert e <= 1.0, (case["name"], e)
        worst = max(worst, e)
        flips += int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        total += got.size
        if dim % 2:
            assert np.array_equal(got[:, -1].view(np.uint32), np.zeros(rows, np.uint32)), case["name"]   # +0.0
    print("embedding: %d of %d elements not bit-equal (cap %d), largest difference %.0f ulp"
          % (flips, total, CR.EMB_FLIP_CAP, worst))
    assert flips <= CR.EMB_FLIP_CAP


# --------------------------------------------------------------------------------------------------------- linear
def _linear(lib, xd, rows, K, wd, bd, O, silu, stride):
    out = nan_buf(rows * stride)
    H.check(lib.ddpm3d_linear(H.ptr(xd), rows, K, H.ptr(wd), H.ptr(bd), O, silu, H.ptr(out), stride, H.stream()))
    assert tail_untouched(out, rows * stride)
    return np_(out[:rows * stride]).reshape(rows, stride)


@pytest.mark.parametrize("rows,K,O", CR.LIN_SHAPES)
def test_linear_element_by_element(rows, K, O):
    lib = H.load()
    for silu in (0, 1):
        case = dict(rows=rows, K=K, O=O, silu=silu)
        x, w, b, small = CR.lin_inputs(case)
        val, _ = CR.linear(x, w, b, silu)
        bar = CR.linear_bar(x, w, b, silu)
        xd, wd, bd = dev(x), dev(w), dev(b)
        got = _linear(lib, xd, rows, K, wd, bd, O, silu, O)
        e = CR.excess(got, val, bar)
        e_small = CR.excess(got[:, small], val[:, small], bar[:, small])
        print("linear rows %d K %d O %d silu %d: |got - ref| / bar %.3f (the small column %.3f)"
              % (rows, K, O, silu, e, e_small))
        assert e <= 1.0, (case, e)
        # out_stride = O + 3: the gap stays NaN, the written columns keep their bits
        wide = _linear(lib, xd, rows, K, wd, bd, O, silu, O + CR.GAP)
        assert np.isnan(wide[:, O:]).all(), case
        assert CR.bits_equal(wide[:, :O], got), case
        assert CR.excess(wide, CR.place(val, O + CR.GAP), np.concatenate([bar, np.ones((rows, CR.GAP))], 1)) <= 1.0
        # a row of the T-row call equals the one-row call on that row
        for i in sorted({0, 7, 8, 999, rows - 1}):
            if i < rows:
                one = _linear(lib, xd[i:i + 1].contiguous(), 1, K, wd, bd, O, silu, O)
                assert CR.bits_equal(one[0], got[i]), (case, i)
        # a NaN in input row 9 makes exactly output row 9 NaN
        if rows > 9:
            bad = x.copy()
            bad[9, K // 2] = np.nan
            poisoned = _linear(lib, dev(bad), rows, K, wd, bd, O, silu, O)
            assert np.isnan(poisoned[9]).all(), case
            others = np.arange(rows) != 9
            assert CR.bits_equal(poisoned[others], got[others]), case


def test_silu_of_the_linear_kernel_on_its_own():
    """K = 1, w = 1, b = 0: every operation behind the SiLU is exact, the output is the kernel's x / (1 + expf(-x))."""
    lib = H.load()
    ref, bar = CR.silu_probe_ref()
    n = len(CR.SILU_PROBE_X)
    got = _linear(lib, dev(CR.SILU_PROBE_X[:, None]), n, 1, dev(np.ones((1, 1))), dev(np.zeros(1)), 1, 1, 1)
    e = CR.excess(got, ref, bar)
    print("SiLU probe: |got - silu(x)| / (5u |silu(x)|) %.3f" % e)
    assert e <= 1.0


def test_silu_tails():
    lib = H.load()
    xs = np.array([-100.0, -88.0, 88.0, 100.0, 0.0, -0.0], dtype=F)
    w = np.array([[0.75], [-3.0]], dtype=F)
    b = np.array([0.0, 0.0], dtype=F)
    got = _linear(lib, dev(xs[:, None]), 6, 1, dev(w), dev(b), 2, 1, 2)
    assert np.isfinite(got).all()
    assert (np.abs(got[0]) <= 2.0 ** -120 * np.abs(w[:, 0])).all(), got[0]
    x100 = xs[3:4, None]
    assert CR.excess(got[3:4], CR.linear(x100, w, b, 1)[0], CR.linear_bar(x100, w, b, 1)) <= 1.0
    assert np.array_equal(got[3], F(100) * w[:, 0])
    assert (got[4:] == 0).all()
    # with a bias, among ordinary operands: finite, and the tails' share is what fp64 says it is
    g = np.random.default_rng(5)
    x = (2.0 * g.standard_normal((3, 70))).astype(F)
    x[:, :6] = xs
    w = (0.05 * g.standard_normal((5, 70))).astype(F)
    b = (0.1 * g.standard_normal(5)).astype(F)
    got = _linear(lib, dev(x), 3, 70, dev(w), dev(b), 5, 1, 5)
    val, _ = CR.linear(x, w, b, 1)
    # -100 and -88 lie outside the range the bar is derived for: their terms may be lost altogether
    lost = np.abs(CR.silu64(xs[:2])).sum() * np.abs(w).max()
    assert lost < 1e-36
    assert np.isfinite(got).all() and CR.excess(got, val, CR.linear_bar(x, w, b, 1) + lost) <= 1.0


# ------------------------------------------------------------------------------------------------ label embedding
@pytest.mark.parametrize("case", CR.LAB_CASES, ids=[c["name"] for c in CR.LAB_CASES])
def test_add_embedding_bit_for_bit(case):
    lib = H.load()
    rows, dim, nc = case["rows"], case["dim"], case["nc"]
    for emb, table, y in CR.lab_launches(case):
        ref = CR.add_embedding(emb, table, y)
        buf = nan_buf(rows * dim)
        buf[:rows * dim] = dev(emb).reshape(-1)
        td, yd = dev(table), torch.from_numpy(y).cuda()
        H.check(lib.ddpm3d_add_embedding(H.ptr(buf), H.ptr(td), H.ptr(yd), rows, dim, nc, H.stream()))
        got = np_(buf[:rows * dim]).reshape(rows, dim)
        assert tail_untouched(buf, rows * dim), (case["name"], y[:5])
        assert CR.bits_equal(got, ref), (case["name"], y[:5])
        bad = (y < 0) | (y >= nc)
        assert CR.bits_equal(got[bad], emb[bad]) and (bad.any() or rows == 1)


# ------------------------------------------------------------------------------------------------------ film_rows
@functools.lru_cache(maxsize=None)
def engine(tag):
    """(engine, the fp32 parameters the path reads, topology, film flag) of cond_ref.MODELS[tag]; only the parameters
    of this path are set from the synthetic recipe, as tests/golden/make_golden_cond.py does."""
    over, seed = CR.MODELS[tag]
    fl = su.sr_model_and_diffusion_defaults()
    fl.update(over)
    with torch.device("cuda"):
        model, _ = su.sr_create_model_and_diffusion(**fl)
    sd = model.state_dict()
    shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    params = CR.cond_params(shapes, seed, synth.synth_param)
    with torch.no_grad():
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(v))
    model.eval()
    return model.engine(), params, model.topology, model.use_scale_shift_norm


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    engine.cache_clear()
    torch.cuda.empty_cache()


def sched_times(tag):
    steps, resp, rescale = CR.SCHEDULES[tag]
    d = su.create_gaussian_diffusion(steps=steps, learn_sigma=True, timestep_respacing=resp, rescale_timesteps=rescale)
    t = d._model_timesteps(torch.arange(d.num_timesteps, device="cuda", dtype=torch.int64))
    return t.to(torch.float32).contiguous()


def _stages(eng, t, y):
    """The calls of UNetEngine.film_rows, one at a time, every buffer NaN-filled first."""
    lib, st, p, R = H.load(), H.stream(), eng.p, t.numel()

    def buf(cols):
        return torch.full((R, cols), float("nan"), device="cuda")

    temb, e1, e2, rows = buf(eng.mc), buf(eng.ted), buf(eng.ted), buf(eng.film_total)
    H.check(lib.ddpm3d_timestep_embedding(H.ptr(t), R, eng.mc, H.ptr(eng.freqs), H.ptr(temb), st))
    H.check(lib.ddpm3d_linear(H.ptr(temb), R, eng.mc, H.ptr(p["time_embed.0.weight"]), H.ptr(p["time_embed.0.bias"]),
                              eng.ted, 0, H.ptr(e1), eng.ted, st))
    H.check(lib.ddpm3d_linear(H.ptr(e1), R, eng.ted, H.ptr(p["time_embed.2.weight"]), H.ptr(p["time_embed.2.bias"]),
                              eng.ted, 1, H.ptr(e2), eng.ted, st))
    e2_pre = e2.clone()
    if y is not None:
        table = p["label_emb.weight"]
        H.check(lib.ddpm3d_add_embedding(H.ptr(e2), H.ptr(table), H.ptr(y), R, eng.ted, table.shape[0], st))
    H.check(lib.ddpm3d_linear(H.ptr(e2), R, eng.ted, H.ptr(eng.emb_w), H.ptr(eng.emb_b), eng.film_total, 1,
                              H.ptr(rows), eng.film_total, st))
    return [np_(v) for v in (temb, e1, e2_pre, e2, rows)]


@pytest.mark.parametrize("sched", list(CR.SCHEDULES))
@pytest.mark.parametrize("tag", list(CR.MODELS))
def test_film_rows_stage_by_stage(tag, sched):
    eng, params, topo, film = engine(tag)
    t = sched_times(sched)
    R = t.numel()
    y = y_np = None
    if "label_emb.weight" in params:
        y_np = CR.golden_labels(R, params["label_emb.weight"].shape[0])
        y = torch.from_numpy(y_np).cuda()
    t_np = np_(t)
    mc = params["time_embed.0.weight"].shape[1]
    assert CR.bits_equal(np_(eng.freqs), CR.freq_table(mc)) and eng.mc == mc
    temb, e1, e2_pre, e2, rows = _stages(eng, t, y)
    # (a) each stage from the GPU's own previous stage
    ref = CR.timestep_embedding(t_np, mc, CR.freq_table(mc))
    fig = {"embedding": CR.excess(temb, ref, CR.ulp_bar(ref))}
    w0, b0, w2, b2 = (params["time_embed.%s" % k] for k in ("0.weight", "0.bias", "2.weight", "2.bias"))
    fig["time_embed.0"] = CR.excess(e1, CR.linear(temb, w0, b0, 0)[0], CR.linear_bar(temb, w0, b0, 0))
    fig["time_embed.2"] = CR.excess(e2_pre, CR.linear(e1, w2, b2, 1)[0], CR.linear_bar(e1, w2, b2, 1))
    if y is not None:
        assert CR.bits_equal(e2, CR.add_embedding(e2_pre, params["label_emb.weight"], y_np))
        assert not CR.bits_equal(e2, e2_pre)
    else:
        assert CR.bits_equal(e2, e2_pre)
    w, b, off = CR.fused_emb_layers(params, topo, film)
    assert off == dict(eng.film_off) and w.shape[0] == eng.film_total == rows.shape[1]
    fig["emb_layers"] = CR.excess(rows, CR.linear(e2, w, b, 1)[0], CR.linear_bar(e2, w, b, 1))
    print("%s / %s, %d rows, |got - ref| / bar per stage: %s"
          % (tag, sched, R, ", ".join("%s %.3f" % kv for kv in fig.items())))
    assert all(v <= 1.0 for v in fig.values()), fig
    # the engine's own call is these calls
    table = eng.film_rows(t, y)
    assert CR.bits_equal(np_(table), rows)
    if y is not None:
        assert not CR.bits_equal(np_(eng.film_rows(t)), rows)
    # (c) row i of the T-row table is the one-row call
    for i in sorted({0, R // 4, R // 2, R - 2, R - 1}):
        one = eng.film_rows(t[i:i + 1].contiguous(), None if y is None else y[i:i + 1].contiguous())
        assert one.shape == (1, eng.film_total) and CR.bits_equal(np_(one)[0], rows[i]), (tag, sched, i)


@pytest.mark.parametrize("tag", list(CR.MODELS))
def test_film_rows_against_the_recorded_reference(golden, tag):
    """(b): the reference implementation's own fp32 run of time_embed, label_emb and every emb_layers."""
    eng, params, topo, film = engine(tag)
    g = golden("cond.npz")
    R = CR.GOLDEN_ROWS[tag]
    t_np = CR.GOLDEN_T[:R]
    y = y_np = None
    if "label_emb.weight" in params:
        y_np = g[tag + "/y"]
        y = torch.from_numpy(y_np).cuda()
    got = np_(eng.film_rows(dev(t_np), y))
    own = CR.film_rows(params, topo, t_np, y_np, film)
    theirs = CR.film_rows(params, topo, t_np, y_np, film, arith="torch")
    expect = g[tag + "/rows"].astype(np.float64)
    bound = own["bound"] + theirs["bound"]
    if not film:                  # the recorded rows are emb_layers' output; the engine's carry the first convs' biases
        cb, fold = CR.conv_bias_fold(params, topo)
        expect, bound = expect + cb[None], bound + fold[None]
    e = CR.excess(got, expect, bound)
    e64 = CR.excess(got, own["rows"], own["bound"])
    print("%s: |film_rows - recorded reference| / bound %.4f; |film_rows - fp64| / own bound %.4f" % (tag, e, e64))
    assert e <= 1.0 and e64 <= 1.0
