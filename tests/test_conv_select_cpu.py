"""
The kernel selection of a conv call without a GPU.

1. tests/golden/conv_select.json, recorded before the selection moved into one place (tests/golden/make_conv_select.py):
   for the descriptor table of tests/conv_select_cases.py every return code, error text, kernel family, ddpm3d_conv_plan
   value and ddpm3d_conv_skip_fused answer is what it was.
2. ddpm3d_conv_kernel_instance against a table of names written from the launchers as they stood then, every one of
   them a kernel symbol of the built library; the three forced issue orders that are not built are named, and absent.
"""

import json
import os
import subprocess
import sys
import tempfile

import pytest

import conv_select_cases as S
from conftest import GOLDEN, ROOT
from guided_diffusion import _hip as H

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_store_hazard as csh  # noqa: E402  (code_objects: the gfx950 code objects of libddpm3d.so)


def test_every_answer_of_the_conv_queries_is_the_recorded_one():
    with open(os.path.join(GOLDEN, "conv_select.json")) as f:
        want = json.load(f)
    blocks, shown = S.table(H.load())
    # the readable subset first: a difference there names its case
    assert list(shown) == list(want["cases"])
    diff = {k: (v, want["cases"][k]) for k, v in shown.items() if v != want["cases"][k]}
    assert not diff, list(diff.items())[:5]
    assert blocks == want["blocks"], [k for k in blocks if blocks[k] != want["blocks"].get(k)]


V64, V32, V16, V8, V4 = (64, 64, 64), (64, 32, 32), (64, 16, 16), (64, 8, 8), (64, 4, 4)
P1, P2, P5 = H.PREC_F16X3, H.PREC_F16, H.PREC_BF16
UP = dict(in_mode=H.IN_UP, kernel_hint=H.HINT_UP_PHASE)
F16SRC = H.IO_SRC0_BF16 | H.IO_HALF_IS_F16
WZ, DIR, PW, SKN = "conv3d_wz_kernel<%s>", "conv3d_kernel<%s>", "conv3d_pw_kernel<%s>", "conv3d_skinny_kernel<%s>"
# (template arguments, conv fields, skip fields or None).  conv3d_wz_kernel<MODE, IL, TX, TY>: MODE 0 f16x3, 1 f16, 2 bf16,
# 3 f16x3 phase, 4 f16x3 skip; conv3d_kernel<PREC, PIPEM, KS, WN, MT, TXL, TYL>; conv3d_pw_kernel<PREC, S16, TXL, TYL, WIDE>;
# conv3d_skinny_kernel<MODE, Cin / 16, source type>
INSTANCES = [
    # plain Winograd-D: 8x4x4 where H % 8 == 0 and D % 4 == 0, else 8x8x2; 4x4x8 below 8x8
    (WZ % "0,4,8,4", S.conv(V64), None), (WZ % "1,0,8,4", S.conv(V64, precision=4), None),
    (WZ % "2,0,8,4", S.conv(V64, precision=6), None), (WZ % "0,4,8,4", S.conv(V32, (256, 256)), None),
    (WZ % "0,4,8,8", S.conv((6, 8, 8)), None), (WZ % "0,4,8,8", S.conv((4, 12, 8)), None),
    (WZ % "1,0,8,8", S.conv((6, 8, 8), precision=4), None), (WZ % "2,0,8,8", S.conv((4, 12, 8), precision=6), None),
    (WZ % "0,4,4,4", S.conv(V4), None), (WZ % "1,0,4,4", S.conv(V4, precision=4), None),
    (WZ % "2,0,4,4", S.conv(V4, precision=6), None), (WZ % "0,4,4,4", S.conv((3, 5, 7)), None),
    # a forced issue order keeps 8x8x2 tiles; it does not reach the 4x4x8 form or the one-MFMA modes' order
    (WZ % "0,0,8,8", S.conv(V64, kernel_hint=S.ORDER(1)), None), (WZ % "0,1,8,8", S.conv(V64, kernel_hint=S.ORDER(2)), None),
    (WZ % "0,2,8,8", S.conv(V64, kernel_hint=S.ORDER(3)), None), (WZ % "0,4,8,8", S.conv(V64, kernel_hint=S.ORDER(5)), None),
    (WZ % "0,4,4,4", S.conv(V4, kernel_hint=S.ORDER(2)), None),
    (WZ % "1,0,8,8", S.conv(V64, precision=4, kernel_hint=S.ORDER(2)), None),
    # the phase variant on the low-resolution grid's tile form; shapes it does not fit run the plain instance
    (WZ % "3,4,8,4", S.conv(V64, **UP), None), (WZ % "3,4,8,4", S.conv(V16, **UP), None),
    (WZ % "3,4,8,8", S.conv((6, 32, 32), **UP), None), (WZ % "3,4,4,4", S.conv(V8, **UP), None),
    (WZ % "3,4,8,4", S.conv(V64, in_mode=H.IN_UP, kernel_hint=H.HINT_UP_PHASE | S.ORDER(2)), None),
    (WZ % "0,4,8,8", S.conv((4, 12, 8), **UP), None), (WZ % "0,4,8,8", S.conv((2, 8, 8), **UP), None),
    (WZ % "0,4,8,4", S.conv(V64, res_mode=H.RES_POOL, res=0x90000, **UP), None),
    # the skip variant on the plain variant's tile form; a pair that does not fuse runs conv2's plain instance
    (WZ % "4,4,8,4", S.conv(V64), S.skip()), (WZ % "4,4,8,8", S.conv((6, 8, 8)), S.skip((128, 128))),
    (WZ % "4,4,4,4", S.conv(V4), S.skip((32, 96))), (WZ % "0,4,8,4", S.conv(V64), S.skip((48,))),
    (WZ % "1,0,8,4", S.conv(V64, precision=4), S.skip()), (WZ % "0,1,8,8", S.conv(V64, kernel_hint=S.ORDER(2)), S.skip()),
    # the direct kernel: each pipe mode, each WN, both tile sizes and kernel sizes, each arithmetic
    (DIR % "1,1,3,4,4,3,3", S.conv(V64, Cout=96, precision=P1), None),
    (DIR % "1,1,3,4,4,3,3", S.conv(V64, Cout=96, precision=P1, in_mode=H.IN_UP), None),
    (DIR % "1,0,3,4,4,3,3", S.conv(V64, Cout=96, precision=P1, in_mode=H.IN_POOL), None),
    (DIR % "1,2,3,4,4,3,3", S.conv(V64, Cout=96, precision=P1, in_mode=H.IN_STRIDE2), None),
    (DIR % "0,0,3,1,1,3,3", S.conv(V64, (1, 1), Cout=32, precision=0), None),
    (DIR % "1,1,3,2,2,3,3", S.conv(V64, Cout=64, precision=P1), None),
    (DIR % "1,1,3,1,1,3,3", S.conv(V64, Cout=32, precision=P1), None),
    (DIR % "1,1,3,4,4,2,2", S.conv(V4, Cout=96, precision=P1), None),
    (DIR % "0,1,3,2,2,2,2", S.conv(V4, Cout=64, precision=0), None),
    (DIR % "0,1,1,4,4,3,3", S.conv(V64, ksize=1, precision=0), None),
    (DIR % "1,1,1,4,4,3,3", S.conv(V64, ksize=1, precision=P1, aff_a=0x20000, aff_b=0x30000), None),
    (DIR % "2,1,3,4,4,3,3", S.conv(V64, precision=P2), None), (DIR % "5,1,3,4,4,3,3", S.conv(V64, precision=P5), None),
    (DIR % "5,1,3,1,1,3,3", S.conv(V64, Cout=2, precision=P5), None),      # bf16 arithmetic on fp32 sources: not skinny
    # the 1x1 GEMM: three arithmetic modes, fp32 and 16-bit sources, both tile sizes
    (PW % "1,0,3,3,1", S.conv(V64, ksize=1, precision=P1), None), (PW % "2,0,3,3,1", S.conv(V64, ksize=1, precision=P2), None),
    (PW % "5,0,3,3,1", S.conv(V64, ksize=1, precision=P5), None),
    (PW % "5,1,3,3,1", S.conv(V64, ksize=1, precision=P5, io_dtype=H.IO_SRC0_BF16), None),
    (PW % "2,1,3,3,1", S.conv(V64, ksize=1, precision=P2, io_dtype=F16SRC), None),
    (PW % "1,0,2,2,1", S.conv(V4, (64, 64), ksize=1, precision=P1), None),
    (PW % "5,1,2,2,1", S.conv(V4, ksize=1, precision=P5, io_dtype=H.IO_SRC0_BF16), None),
    (PW % "2,0,2,2,1", S.conv(V4, ksize=1, precision=P2), None),
    # the skinny kernel: Cin 32, 64, 128 and each source type
    (SKN % "0,2,0", S.conv(V64, (32, 0), Cout=2, precision=P1), None),
    (SKN % "0,4,0", S.conv(V64, (64, 0), Cout=2, precision=P1), None),
    (SKN % "0,8,0", S.conv(V64, Cout=1, precision=P1), None), (SKN % "1,8,0", S.conv(V64, Cout=2, precision=P2), None),
    (SKN % "1,4,2", S.conv(V64, (64, 0), Cout=2, precision=P2, io_dtype=F16SRC), None),
    (SKN % "1,2,2", S.conv(V4, (32, 0), Cout=2, precision=P2, io_dtype=F16SRC), None),
    (SKN % "2,8,1", S.conv(V64, Cout=2, precision=P5, io_dtype=H.IO_SRC0_BF16), None),
    (SKN % "2,2,1", S.conv(V64, (32, 0), Cout=2, precision=P5, io_dtype=H.IO_SRC0_BF16), None),
]
NOT_BUILT = [(WZ % ("0,%d,8,8" % il), S.conv(V64, kernel_hint=S.ORDER(il + 1)), None) for il in (3, 5, 6)]


def _instance(fields, sk):
    d, s = S.build(fields, sk)
    return H.conv_instance(d, s)


@pytest.mark.parametrize("want,fields,sk", INSTANCES + NOT_BUILT,
                         ids=["%s %s" % (w, S.case_id(f, s)) for w, f, s in INSTANCES + NOT_BUILT])
def test_the_instance_query_names_the_kernel_the_launcher_ran(want, fields, sk):
    assert _instance(fields, sk) == want


def test_the_instance_query_refuses_what_the_family_query_refuses():
    lib = H.load()
    for fields, sk in [(S.conv(Cout=96), None), (S.conv(ksize=2), None), (S.conv(kernel_hint=H.HINT_UP_PHASE), None),
                       (S.conv(res_mode=H.RES_SAME, res=0x90000), S.skip()), (S.conv(), S.skip(C0=0))]:
        rec = S.record(lib, fields, sk)
        with pytest.raises(H.Ddpm3dError) as e:
            _instance(fields, sk)
        if sk is None:
            assert (e.value.code, str(e.value)) == (rec[0], "ddpm3d error %d: %s" % (rec[0], rec[1]))
        else:
            assert e.value.code == H.E_INVAL and "conv3d_skip" in str(e.value) and rec[5] == 0
    d, _ = S.build(S.conv(), None)
    assert lib.ddpm3d_conv_kernel_instance(d, None, None, 0) == H.E_INVAL
    short = (H.C.c_char * 8)()
    assert lib.ddpm3d_conv_kernel_instance(d, None, short, 8) == H.E_INVAL


@pytest.fixture(scope="module")
def built():
    """the conv kernels of the library's gfx950 code objects, spelled like the instance query"""
    readelf = os.path.join(csh.LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf here")
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        for f in csh.code_objects(H.LIB_PATH, tmp):
            syms = subprocess.run([readelf, "--symbols", "--wide", f], capture_output=True, text=True, check=True).stdout
            names |= {S.instance_of_symbol(ln.split()[-1]) for ln in syms.splitlines() if " FUNC " in ln and "conv3d" in ln}
    return names - {None}


def test_trace_names_and_symbols_are_spelled_like_the_query():
    assert S.instance_of("void conv3d_wz_kernel<0, 4, 8, 4>(ConvK)") == "conv3d_wz_kernel<0,4,8,4>"
    assert S.instance_of("conv3d_wz_kernel<0, 4, 8, 4>(ConvK) [clone .kd]") == "conv3d_wz_kernel<0,4,8,4>"
    assert S.instance_of("void (anonymous namespace)::conv3d_pw_kernel<1, 0, 3, 3, true>(ConvK)") == "conv3d_pw_kernel<1,0,3,3,1>"
    assert S.instance_of("(anonymous namespace)::conv3d_skinny_kernel<0, 8, 0>(ConvK, int, int)") == "conv3d_skinny_kernel<0,8,0>"
    assert S.instance_of("conv_splitk_reduce_kernel(ConvK)") is None
    assert S.instance_of_symbol("_Z16conv3d_wz_kernelILi0ELi4ELi8ELi4EEv5ConvK") == "conv3d_wz_kernel<0,4,8,4>"
    assert S.instance_of_symbol("_ZN12_GLOBAL__N_116conv3d_pw_kernelILi1ELi0ELi3ELi3ELb1EEEv5ConvK") == "conv3d_pw_kernel<1,0,3,3,1>"
    assert S.instance_of_symbol("_ZN12_GLOBAL__N_120conv3d_skinny_kernelILi0ELi8ELi0EEEv5ConvKii") == "conv3d_skinny_kernel<0,8,0>"
    assert S.instance_of_symbol("_Z25conv_splitk_reduce_kernel5ConvK") is None


def test_every_expected_instance_is_a_kernel_of_the_built_library(built):
    assert len(built) >= 18
    missing = sorted({w for w, _, _ in INSTANCES} - built)
    assert not missing, (missing, sorted(built))
    # the Winograd-D kernel is built in exactly the eighteen forms the table of DESIGN 1.2 lists
    wz = sorted(n for n in built if n.startswith("conv3d_wz_kernel<"))
    assert wz == sorted(WZ % a for a in ["0,0,8,8", "0,1,8,8", "0,2,8,8"] + [
        "%d,%d,%s" % (m, 0 if m in (1, 2) else 4, t) for m in range(5) for t in ("8,8", "8,4", "4,4")])
    # forced orders 3, 5, 6: named by the query, not built -- their launch fails with hipErrorInvalidValue as before
    assert not {w for w, _, _ in NOT_BUILT} & built
