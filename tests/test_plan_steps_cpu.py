"""
The UNet planner (csrc/unet_plan.hip) is host code: on descriptions built from the topology with stand-in addresses,
against an arena that is never dereferenced, it must produce the step lists recorded in tests/golden/plan_steps.json
(recorded while engine.py still planned the forward itself, and proven equal to its lists then); and it must refuse a
malformed description before it indexes anything.
"""

import ctypes as C
import json
import os

import pytest

import guided_diffusion._hip as H
import plan_steps as P

ARENA = 1 << 44
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_steps.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _plan(case, desc=None, keep=None):
    lib = H.load()
    with P.switches(case):
        model, _ = P.build(case)
        if desc is None:
            desc, keep = P.host_desc(model, P.fake_addresses())
        handle, need, pl = P.planner_steps(lib, desc, case.shape, ARENA)
    return lib, handle, need, pl, model._planar()


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_planner_gives_the_recorded_step_list(golden, name):
    lib, handle, need, pl, planar = _plan(P.CASES[name])
    try:
        sig = P.signature(pl, planar)
        if name in P.SMALL:         # the lists themselves, so that a difference names its step
            with open(GOLDEN.replace(".json", "_small.json")) as f:
                want = json.load(f)[name]
            for k, (a, b) in enumerate(zip(json.loads(json.dumps(sig)), want)):
                assert a == b, "step %d" % k
            assert len(sig) == len(want)
        got, want = P.digest(sig, P.meta(pl)), golden[name]
        assert got == {k: want[k] for k in got}
    finally:
        lib.ddpm3d_unet_plan_destroy(handle)


def _tiny_desc():
    case = P.CASES["tiny"]
    model, _ = P.build(case)
    desc, keep = P.host_desc(model, P.fake_addresses())
    return case, model, desc, keep


def _refused(desc, shape, what):
    lib = H.load()
    N, D, Hh, W = P.ndhw(shape)
    assert lib.ddpm3d_unet_plan_bytes(C.byref(desc), N, D, Hh, W) == 0
    assert what in lib.ddpm3d_unet_last_error().decode()
    handle = C.c_void_p()
    assert lib.ddpm3d_unet_plan_create(C.byref(desc), N, D, Hh, W, ARENA, 1 << 40, C.byref(handle)) == H.E_INVAL
    assert what in lib.ddpm3d_unet_last_error().decode() and not handle.value


def test_block_table_that_covers_more_layers_than_there_are_is_refused():
    case, _, desc, keep = _tiny_desc()
    desc.output_block_layers[desc.n_output_blocks - 1] += 1     # the loops would index past `layers`
    _refused(desc, case.shape, "block sizes cover")
    desc.output_block_layers[desc.n_output_blocks - 1] -= 2
    _refused(desc, case.shape, "block sizes cover")
    desc.output_block_layers[desc.n_output_blocks - 1] = -1
    _refused(desc, case.shape, "block sizes cover")


def test_more_output_blocks_than_skips_are_refused():
    case, _, desc, keep = _tiny_desc()
    sizes = [desc.output_block_layers[b] for b in range(desc.n_output_blocks)]
    assert desc.n_output_blocks == desc.n_input_blocks + 1
    b = next(i for i, s in enumerate(sizes) if s == 2)
    sizes[b:b + 1] = [1, 1]                                     # the same layers, one block more than the skip stack holds
    arr = (C.c_int32 * len(sizes))(*sizes)
    desc.n_output_blocks, desc.output_block_layers = len(sizes), arr
    _refused(desc, case.shape, "skip stack")


IN_GEOMETRY = {H.IN_SAME: (1, 1), H.IN_POOL: (2, 2), H.IN_UP: (0.5, 0.5), H.IN_STRIDE2: (2, 2)}


def _check_liveness(pl):
    """From the step list alone.  (1) Live intervals: an activation lives from the step that writes its buffer to the
    last step that reads it before the buffer is written again; the byte ranges of activations whose intervals overlap
    are pairwise disjoint.  (2) Two tensors planned at the SAME offset cannot be told apart by intervals (the second
    write just ends the first interval), so also: no step writes over a tensor it reads (the residual, read and
    written voxel by voxel, excepted), and every read sees the shape and storage the buffer's last writer gave it."""
    shape, live, done = {}, {}, []              # per pointer: (C, D, H, W, 16-bit) / [pointer, bytes, first, last]

    def write(k, N, ptr, C, D, Hh, W, half):
        if ptr in live:
            done.append(live[ptr])
        shape[ptr] = (C, D, Hh, W, half)
        live[ptr] = [ptr, N * C * D * Hh * W * (2 if half else 4), k, k]

    def read(k, ptr):
        if ptr in live:
            live[ptr][3] = k
        return shape.get(ptr)

    for k, (fn, args) in enumerate(pl.steps):
        name = fn.__name__
        if name in ("ddpm3d_conv3d", "ddpm3d_conv3d_skip"):
            d = args[0]._obj
            reads = []
            if d.in_mode != H.IN_PLANAR2:
                fy, fx = IN_GEOMETRY[d.in_mode]
                reads += [(d.src0, d.C0, d.D, d.H * fy, d.W * fx, bool(d.io_dtype & H.IO_SRC0_BF16))]
                if d.C1:
                    reads += [(d.src1, d.C1, d.D, d.H * fy, d.W * fx, bool(d.io_dtype & H.IO_SRC1_BF16))]
            if name == "ddpm3d_conv3d_skip":
                sk = args[1]._obj
                reads += [(sk.src0, sk.C0, d.D, d.H, d.W, bool(sk.io_dtype & H.IO_SRC0_BF16))]
                if sk.C1:
                    reads += [(sk.src1, sk.C1, d.D, d.H, d.W, bool(sk.io_dtype & H.IO_SRC1_BF16))]
            for r in reads:
                assert r[0] != d.out, "a conv writes over its own input"
                assert read(k, r[0]) == r[1:], "a conv reads a buffer another tensor was planned into"
            if d.res_mode != H.RES_NONE:
                fy, fx = {H.RES_SAME: (1, 1), H.RES_POOL: (2, 2), H.RES_UP: (0.5, 0.5)}[d.res_mode]
                assert read(k, d.res) == (d.Cout, d.D, d.H * fy, d.W * fx, bool(d.io_dtype & H.IO_RES_BF16))
            if d.out:
                write(k, d.N, d.out, d.Cout, d.D, d.H, d.W, bool(d.io_dtype & H.IO_OUT_BF16))
        elif name == "ddpm3d_pool_act":
            src, dst, (N, D, Hh, W, Cn), io = args[0], args[10], args[5:10], args[11]
            assert src != dst and read(k, src) == (Cn, D, 2 * Hh, 2 * W, bool(io & H.IO_SRC0_BF16))
            write(k, N, dst, Cn, D, Hh, W, False)
        elif name == "ddpm3d_attention_p":
            qkv, dst, (N, T, heads, ch) = args[0], args[9], args[1:5]
            w = read(k, qkv)
            assert qkv != dst and w is not None and w[0] == 3 * heads * ch and w[1] * w[2] * w[3] == T and not w[4]
            write(k, N, dst, heads * ch, w[1], w[2], w[3], False)
    done += live.values()
    assert len(done) > 3
    for i, (p0, n0, a0, b0) in enumerate(done):
        for p1, n1, a1, b1 in done[i + 1:]:
            if p0 != p1 and a0 <= b1 and a1 <= b0:
                assert p0 + n0 <= p1 or p1 + n1 <= p0, "two live activations overlap in the arena"


@pytest.mark.parametrize("name", ["tiny", "tiny attention", "tiny bf16", "published"])
def test_recorded_cases_pass_the_liveness_check(name):
    lib, handle, need, pl, planar = _plan(P.CASES[name])
    try:
        _check_liveness(pl)
    finally:
        lib.ddpm3d_unet_plan_destroy(handle)


def test_description_without_a_middle_block_releases_its_shared_tensor_once():
    """n_middle_layers == 0: the first output block's input and its skip are ONE tensor; released twice, its buffer
    would be handed to the next two activations of that size at once.  The smallest such network: the first conv,
    then one output block of the tiny network's last ResBlock (64 -> 32 over [h, h]) and its first (32 -> 32, whose
    two activations have the size of h)."""
    case, model, desc, keep = _tiny_desc()
    lib = H.load()
    layers = [desc.layers[desc.n_layers - 1], desc.layers[0]]
    assert (layers[0].conv1.Cin, layers[0].conv2.Cout, layers[1].conv1.Cin, layers[1].conv2.Cout) == (64, 32, 32, 32)
    arr = (H.Layer * 2)(*layers)
    sizes = (C.c_int32 * 1)(2)
    desc.n_layers, desc.layers = 2, arr
    desc.n_input_blocks = desc.n_middle_layers = 0
    desc.n_output_blocks, desc.output_block_layers = 1, sizes
    handle, need, pl = P.planner_steps(lib, desc, case.shape, ARENA)
    try:
        assert [fn.__name__ for fn, _ in pl.steps].count("ddpm3d_gn_finalize") == 5
        _check_liveness(pl)
    finally:
        lib.ddpm3d_unet_plan_destroy(handle)


def test_step_query_counts_and_respects_the_capacity():
    lib, handle, need, pl, planar = _plan(P.CASES["tiny additive"])
    try:
        n = lib.ddpm3d_unet_plan_steps(handle, None, 0)
        assert n == len(pl.steps) > 5
        recs = (H.PlanStep * 5)()
        for r in recs:
            r.kind = -7
        assert lib.ddpm3d_unet_plan_steps(handle, recs, 3) == n
        assert [r.kind for r in recs[:3]] == [H.STEP_ABSMAX, H.STEP_CONV, H.STEP_FINALIZE]
        assert [r.kind for r in recs[3:]] == [-7, -7]
        assert lib.ddpm3d_unet_plan_steps(None, recs, 5) < 0
        # the role flags of the additive-embedding network: conv1 of every ResBlock takes its bias from the film row
        full = (H.PlanStep * n)()
        lib.ddpm3d_unet_plan_steps(handle, full, n)
        assert full[1].flags == H.STEP_X | H.STEP_LOW_RES and full[n - 1].flags == H.STEP_OUT
        assert sum(1 for r in full if r.flags & H.STEP_FILM_BIAS) == len(pl.bias_patches) > 0
        assert not any(r.flags & H.STEP_FILM for r in full)
    finally:
        lib.ddpm3d_unet_plan_destroy(handle)
