"""
The descriptor table behind tests/golden/conv_select.json: what the conv entries answer, without a GPU, for a
deterministic set of ddpm3d_conv_desc / ddpm3d_conv_skip pairs on made-up (never dereferenced) addresses -- the return
code and error text, the kernel family, ddpm3d_conv_plan's three values and ddpm3d_conv_skip_fused.

A case is (fields of the conv descriptor, fields of the skip descriptor or None); `cases()` yields them block by block,
`record()` asks the library.  tests/golden/make_conv_select.py writes the golden from this table and
tests/test_conv_select_cpu.py replays it.
"""

import ctypes as C
import hashlib
import itertools
import json

from guided_diffusion import _hip as H

VOLUMES = [(64, 64, 64), (64, 32, 32), (64, 16, 16), (64, 8, 8), (64, 4, 4), (2, 8, 8), (6, 8, 8), (4, 12, 8), (3, 5, 7),
           (1, 1, 1)]
COUTS = [1, 2, 32, 64, 96, 128, 256, 384]
# (C0, C1): Cin 2 is the planar input; every other Cin alone and as a concat, plus splits that are not whole 32-blocks
CINS = [(1, 1), (16, 0), (32, 0), (16, 16), (128, 0), (64, 64), (96, 32), (48, 80), (512, 0), (256, 256), (1024, 0),
        (512, 512)]
ORDER = lambda o: o << H.HINT_WZ_ORDER_SHIFT      # noqa: E731
SPLIT = lambda s: s << H.HINT_SPLITK_SHIFT        # noqa: E731
HINTS = [0, H.HINT_UP_PHASE] + [ORDER(o) for o in range(1, 8)] + [SPLIT(2), SPLIT(17), H.HINT_WSTAT_OFF, H.HINT_WSTAT_ON,
         H.HINT_WSTAT_OFF | H.HINT_WSTAT_ON, H.HINT_UP_PHASE | ORDER(2), H.HINT_UP_PHASE | SPLIT(2), ORDER(3) | SPLIT(2)]

BASE = dict(N=1, D=8, H=8, W=8, Cin=128, Cout=128, ksize=3, in_mode=H.IN_SAME, src0=0x10000, src1=0, C0=128, C1=0,
            aff_a=0, aff_b=0, act=H.ACT_NONE, precision=H.PREC_F16X3_WZ, w_packed=0x40000, bias=0x50000, bias_stride_n=0,
            res_mode=H.RES_NONE, res=0, out=0x60000, out_layout=H.OUT_NDHWC, stats_rows=0, stats=0,
            workspace=0x1000000, workspace_bytes=1 << 40, kernel_hint=0, in_bound_count=1, in_bound=0x70000,
            in_bound_stride=1, io_dtype=0)
SKIP_BASE = dict(src0=0x80000, src1=0, C0=64, C1=0, w_packed=0xA0000, bias=0xB0000, in_bound=0x70004, in_bound_count=1,
                 in_bound_stride=1, io_dtype=0)


def conv(vol=None, cin=None, **kw):
    """overrides of BASE; vol = (D, H, W), cin = (C0, C1) (Cin 2: the planar input)"""
    f = {}
    if vol is not None:
        f.update(D=vol[0], H=vol[1], W=vol[2])
    if cin is not None:
        f.update(Cin=cin[0] + cin[1], C0=cin[0], C1=cin[1], src1=0x20000 if cin[1] else 0)
        if cin == (1, 1):
            f.update(in_mode=H.IN_PLANAR2)
    f.update(kw)
    return f


def skip(cx=(64,), **kw):
    f = dict(C0=cx[0])
    if len(cx) > 1:
        f.update(C1=cx[1], src1=0x90000)
    f.update(kw)
    return f


# ---- single faults (the pairs of them record which refusal wins)
FAULTS = [dict(N=0), dict(D=-1), dict(Cout=0), dict(ksize=2), dict(precision=7), dict(precision=-1), dict(C0=112),
          dict(in_mode=9), dict(in_mode=H.IN_STRIDE2, ksize=1), dict(Cin=24, C0=24), dict(C0=8, C1=120, src1=0x20000),
          dict(src0=0x10004), dict(src1=0x20008), dict(in_mode=H.IN_UP, H=7), dict(aff_a=0x20000), dict(aff_a=0x20004, aff_b=0x30000),
          dict(w_packed=0x40004), dict(res_mode=5), dict(res_mode=H.RES_SAME), dict(res_mode=H.RES_UP, res=0x90000, W=7),
          dict(bias_stride_n=-1), dict(out_layout=2), dict(kernel_hint=SPLIT(63)), dict(Cout=96),
          dict(kernel_hint=H.HINT_UP_PHASE), dict(io_dtype=0x40), dict(io_dtype=H.IO_OUT_BF16, out_layout=H.OUT_NCDHW),
          dict(in_bound=0), dict(in_bound_count=65), dict(stats=0xC0000, stats_rows="rows+1"), dict(stats=0xC0008, stats_rows="rows"),
          dict(stats=0xC0000, stats_rows="rows", out_layout=H.OUT_NCDHW), dict(N=4096, D=64, H=64, W=64),
          dict(D=2048, H=512, W=512), dict(N=1 << 20, D=64, H=64, W=64, Cin=16, C0=16)]
FAULT_BASES = [dict(), dict(precision=H.PREC_F16X3, ksize=1), dict(precision=H.PREC_F32, Cin=2, C0=1, C1=1, src1=0x20000,
                                                                  in_mode=H.IN_PLANAR2, Cout=32)]


def cases():
    """yields (block, shown in full, conv fields, skip fields or None)"""
    for prec, ks in itertools.product(range(7), (1, 3)):
        blk = "shape/p%d_k%d" % (prec, ks)
        for vol, cout, cin in itertools.product(VOLUMES, COUTS, CINS):
            yield blk, cout == 128 and cin == (128, 0), conv(vol, cin, Cout=cout, ksize=ks, precision=prec), None
        for n, vol, cout, cin in itertools.product((2, 8), VOLUMES[3:6], (128, 384), ((512, 0), (512, 512))):
            yield blk, False, conv(vol, cin, N=n, Cout=cout, ksize=ks, precision=prec), None
    for prec in range(7):
        blk = "modes/p%d" % prec
        for in_mode, res_mode, ks, vol, (cout, cin), aff in itertools.product(
                range(-1, 6), range(-1, 5), (1, 3), (VOLUMES[0], VOLUMES[4], VOLUMES[6], VOLUMES[7], VOLUMES[8]),
                ((128, (128, 0)), (2, (32, 0)), (64, (32, 0)), (256, (64, 64))), (0, 1)):
            f = conv(vol, (1, 1) if in_mode == H.IN_PLANAR2 else cin, Cout=cout, ksize=ks, precision=prec, res_mode=res_mode,
                     res=0x90000 if res_mode else 0)
            f.update(in_mode=in_mode)
            if aff:
                f.update(aff_a=0x20000, aff_b=0x30000, act=H.ACT_SILU)
            yield blk, ks == 3 and cout == 128 and vol == VOLUMES[6] and not aff and res_mode in (0, 2), f, None
    for prec in range(7):
        blk = "io/p%d" % prec
        for io, layout, ks, (cout, cin), vol, stats in itertools.product(
                list(range(32)) + [32, 64], (H.OUT_NDHWC, H.OUT_NCDHW), (1, 3),
                ((2, (32, 0)), (2, (64, 0)), (2, (128, 0)), (1, (128, 0)), (128, (128, 0)), (128, (64, 64)), (2, (256, 0)),
                 (2, (16, 16))), (VOLUMES[0], VOLUMES[4]), (0, 1)):
            f = conv(vol, cin, Cout=cout, ksize=ks, precision=prec, io_dtype=io, out_layout=layout)
            if stats:
                f.update(stats=0xC0000, stats_rows="rows")
            yield blk, vol == VOLUMES[0] and layout == 0 and cin == (128, 0) and io in (0, 1, 17, 4) and not stats, f, None
    hint_vols = VOLUMES + [(64, 16, 8), (6, 32, 32), (8, 16, 16), (4, 16, 24)]
    for prec in range(7):
        blk = "hints/p%d" % prec
        for hint, in_mode, res_mode, ks, vol, (cout, cin) in itertools.product(
                HINTS, (H.IN_SAME, H.IN_UP), (H.RES_NONE, H.RES_POOL), (1, 3), hint_vols,
                ((128, (128, 0)), (128, (32, 0)), (256, (256, 256)), (64, (64, 0)), (384, (512, 512)))):
            f = conv(vol, cin, Cout=cout, ksize=ks, precision=prec, kernel_hint=hint, in_mode=in_mode, res_mode=res_mode,
                     res=0x90000 if res_mode else 0)
            yield blk, prec == 3 and ks == 3 and cout == 128 and cin == (128, 0) and res_mode == 0 and vol in (
                (64, 64, 64), (64, 8, 8), (6, 32, 32), (4, 12, 8)), f, None
    variants = [(dict(), dict()), (dict(io_dtype=H.IO_OUT_BF16), dict()), (dict(), dict(io_dtype=H.IO_SRC0_BF16)),
                (dict(kernel_hint=ORDER(2)), dict()), (dict(kernel_hint=SPLIT(2)), dict()),
                (dict(kernel_hint=H.HINT_UP_PHASE), dict()), (dict(), dict(bias=0xB0004)), (dict(in_mode=H.IN_UP), dict()),
                (dict(), dict(C0=0)), (dict(res_mode=H.RES_SAME, res=0x90000), dict()), (dict(ksize=1), dict()),
                (dict(out_layout=H.OUT_NCDHW), dict()), (dict(), dict(w_packed=0xA0004)), (dict(), dict(in_bound=0))]
    for prec in range(7):
        blk = "skip/p%d" % prec
        for vol, cout, cx, (dv, sv) in itertools.product(
                VOLUMES, (128, 256, 64, 96), ((64,), (128, 128), (32, 96), (48,), (16, 48), (512, 512)), variants):
            f = conv(vol, (cout, 0), Cout=cout, precision=prec, aff_a=0x20000, aff_b=0x30000, act=H.ACT_SILU)
            f.update(dv)
            s = skip(cx)
            s.update(sv)
            yield blk, prec == 3 and cout == 128 and cx in ((64,), (48,)) and vol in VOLUMES[3:8], f, s
    for b, base in enumerate(FAULT_BASES):
        for fault in FAULTS:
            yield "refusals/one", True, dict(base, **fault), None
        for i, j in itertools.combinations(range(len(FAULTS)), 2):
            if set(FAULTS[i]) & set(FAULTS[j]):
                continue
            yield "refusals/two", b == 0 and i < 4, dict(base, **FAULTS[i], **FAULTS[j]), None


def case_id(fields, sk):
    s = " ".join("%s=%s" % (k, ("%#x" % v) if isinstance(v, int) and v > 0xFFFF else v) for k, v in fields.items())
    if sk is not None:
        s += " | " + " ".join("%s=%s" % (k, ("%#x" % v) if v > 0xFFFF else v) for k, v in sk.items())
    return s


def build(fields, sk):
    """the ctypes descriptors of a case (stats_rows "rows" / "rows+1": what ddpm3d_conv_plan says for the rest)"""
    d = H.ConvDesc()
    want_rows = None
    for k, v in dict(BASE, **fields).items():
        if k == "stats_rows" and isinstance(v, str):
            want_rows = v
            continue
        setattr(d, k, v)
    if want_rows is not None:
        stats, d.stats = d.stats, 0
        rows = C.c_int(0)
        H.load().ddpm3d_conv_plan(C.byref(d), C.byref(rows), None, None)
        d.stats, d.stats_rows = stats, rows.value + (1 if want_rows == "rows+1" else 0)
    s = None
    if sk is not None:
        s = H.ConvSkip()
        for k, v in dict(SKIP_BASE, **sk).items():
            setattr(s, k, v)
    return d, s


def record(lib, fields, sk):
    """[family rc, its error text, family, plan rc, [rows, workspace bytes, split] or None, fused or None]"""
    d, s = build(fields, sk)
    name = C.create_string_buffer(96)
    rc = lib.ddpm3d_conv_kernel_family(C.byref(d), name, 96)
    err = lib.ddpm3d_last_error().decode() if rc else ""
    rows, ws, split = C.c_int(-1), C.c_size_t(0), C.c_int(-1)
    prc = lib.ddpm3d_conv_plan(C.byref(d), C.byref(rows), C.byref(ws), C.byref(split))
    fused = lib.ddpm3d_conv_skip_fused(C.byref(d), C.byref(s)) if s is not None else None
    return [rc, err, name.value.decode() if rc == 0 else "", prc, [rows.value, ws.value, split.value] if prc == 0 else None,
            fused]


def table(lib):
    """({block: {"cases": n, "sha256": digest of its records in order}}, {case id: record} of the cases shown in full)"""
    blocks, shown = {}, {}
    for blk, show, fields, sk in cases():
        rec = record(lib, fields, sk)
        cid = case_id(fields, sk)
        b = blocks.setdefault(blk, [0, hashlib.sha256()])
        b[0] += 1
        b[1].update((cid + "\t" + json.dumps(rec, separators=(",", ":")) + "\n").encode())
        if show:
            shown[blk + ": " + cid] = rec
    return {k: {"cases": n, "sha256": h.hexdigest()} for k, (n, h) in blocks.items()}, shown


def instance_of(traced):
    """a kernel name as a trace or a demangler prints it -> ddpm3d_conv_kernel_instance's spelling: return type,
    "(anonymous namespace)::", parameter list and blanks dropped, true / false as 1 / 0; None: not a template kernel"""
    import re
    m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?(\w+<[^>()]*>)(?:\(.*\))?(?: \[clone [^\]]*\])?$", traced.strip())
    if not m:
        return None
    return m.group(1).replace(" ", "").replace("true", "1").replace("false", "0")


def instance_of_symbol(mangled):
    """an Itanium-mangled kernel symbol of the code objects -> the same spelling (integer and bool template arguments
    only, which is all the conv kernels have); None: not such a symbol"""
    import re
    m = re.match(r"^_Z(?:N12_GLOBAL__N_1)?(\d+)", mangled)
    if not m:
        return None
    n, at = int(m.group(1)), m.end()
    name, rest = mangled[at:at + n], mangled[at + n:]
    a = re.match(r"^I((?:L[ib]n?\d+E)+)E", rest)
    if not a:
        return None
    args = [("-" if g[0] else "") + g[1] for g in re.findall(r"L[ib](n?)(\d+)E", a.group(1))]
    return "%s<%s>" % (name, ",".join(args))
