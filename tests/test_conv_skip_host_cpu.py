"""
ddpm3d_conv3d_skip without a GPU: the ctypes mirror of ddpm3d_conv_skip has the header's layout, the entry refuses bad
arguments on the host (DDPM3D_EINVAL before any HIP call), and ddpm3d_conv_skip_fused -- the library's own routing
decision -- says "fused" for the f16x3 Winograd-D ResBlock tails and "two calls" for everything the fused form does
not cover.  ABI version and sizeof(ddpm3d_conv_desc) are untouched (additive within ABI 13).
"""

import ctypes as C
import os
import subprocess
import tempfile

from conftest import ROOT
from guided_diffusion import _hip as H


def test_conv_skip_struct_layout_matches_header():
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "ddpm3d.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(ddpm3d_conv_skip), offsetof(ddpm3d_conv_skip, C0),
           offsetof(ddpm3d_conv_skip, w_packed), offsetof(ddpm3d_conv_skip, bias), offsetof(ddpm3d_conv_skip, in_bound),
           offsetof(ddpm3d_conv_skip, in_bound_count), offsetof(ddpm3d_conv_skip, io_dtype), sizeof(ddpm3d_conv_desc),
           DDPM3D_ABI_VERSION);
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "layout.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "layout")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    S = H.ConvSkip
    assert got == [C.sizeof(S), S.C0.offset, S.w_packed.offset, S.bias.offset, S.in_bound.offset,
                   S.in_bound_count.offset, S.io_dtype.offset, C.sizeof(H.ConvDesc), H.ABI_VERSION]
    assert C.sizeof(H.ConvDesc) == 176 and H.ABI_VERSION == 13


def _pair(D=8, Hh=8, W=8, Cout=128, Cx=(64,), prec=H.PREC_F16X3_WZ):
    """a ResBlock tail on made-up (never dereferenced) 256-byte aligned addresses"""
    d = H.ConvDesc()
    d.N, d.D, d.H, d.W, d.Cin, d.Cout, d.ksize, d.in_mode = 1, D, Hh, W, Cout, Cout, 3, H.IN_SAME
    d.src0, d.C0 = 0x10000, Cout
    d.aff_a, d.aff_b, d.act = 0x20000, 0x30000, H.ACT_SILU
    d.precision, d.w_packed, d.bias, d.out = prec, 0x40000, 0x50000, 0x60000
    d.in_bound, d.in_bound_count, d.in_bound_stride = 0x70000, 32, 2
    d.workspace, d.workspace_bytes = 0x1000000, 1 << 40
    sk = H.ConvSkip()
    sk.src0, sk.C0 = 0x80000, Cx[0]
    if len(Cx) > 1:
        sk.src1, sk.C1 = 0x90000, Cx[1]
    sk.w_packed, sk.bias = 0xA0000, 0xB0000
    sk.in_bound, sk.in_bound_count, sk.in_bound_stride = 0x70004, 32, 2
    return d, sk


def _fused(d, sk):
    return H.load().ddpm3d_conv_skip_fused(C.byref(d), C.byref(sk))


def test_the_library_decides_where_the_fused_form_runs():
    assert _fused(*_pair()) == 1
    assert _fused(*_pair(Cx=(128, 128))) == 1
    assert _fused(*_pair(D=9, Hh=4, W=6, Cout=256, Cx=(32, 96))) == 1
    # everything else runs as the two shipped calls
    assert _fused(*_pair(prec=H.PREC_F16X3)) == 0                      # conv2 not on the Winograd-D form
    assert _fused(*_pair(prec=H.PREC_F16_WZ)) == 0 and _fused(*_pair(prec=H.PREC_BF16_WZ)) == 0
    assert _fused(*_pair(prec=H.PREC_F32)) == 0
    assert _fused(*_pair(Cx=(48,))) == 0                              # not whole 32-channel blocks
    assert _fused(*_pair(Cx=(16, 48))) == 0
    d, sk = _pair()
    d.io_dtype = H.IO_OUT_BF16
    assert _fused(d, sk) == 0                                         # 16-bit I/O
    d, sk = _pair()
    sk.io_dtype = H.IO_SRC0_BF16
    assert _fused(d, sk) == 0
    d, sk = _pair()
    d.kernel_hint = 2 << H.HINT_WZ_ORDER_SHIFT                        # a forced issue order has no fused instantiation
    assert _fused(d, sk) == 0
    d, sk = _pair()
    sk.bias = 0xB0004                                                 # the reduce launch reads the bias 16 bytes wide
    assert _fused(d, sk) == 0
    # a forced split keeps the fused form (conv2's own split factor, rows and workspace)
    d, sk = _pair()
    d.kernel_hint = 2 << H.HINT_SPLITK_SHIFT
    assert _fused(d, sk) == 1 and H.conv_plan(d)[2] == 2


def test_conv3d_skip_refuses_bad_arguments_on_the_host():
    lib = H.load()
    d, sk = _pair()
    assert lib.ddpm3d_conv3d_skip(None, C.byref(sk), None) == H.E_INVAL
    assert lib.ddpm3d_conv3d_skip(C.byref(d), None, None) == H.E_INVAL
    assert lib.ddpm3d_conv_skip_fused(None, None) == 0
    bad = [("res_mode", H.RES_SAME), ("out_layout", H.OUT_NCDHW), ("ksize", 1), ("N", 0), ("out", 0), ("bias", 0)]
    for field, value in bad:
        d, sk = _pair()
        setattr(d, field, value)
        assert lib.ddpm3d_conv3d_skip(C.byref(d), C.byref(sk), None) == H.E_INVAL, field
    for field, value in [("C0", 0), ("C0", 24), ("C1", -16), ("io_dtype", H.IO_OUT_BF16), ("src0", 0), ("w_packed", 0),
                         ("bias", 0), ("in_bound", 0), ("w_packed", 0xA0004)]:
        d, sk = _pair()
        setattr(sk, field, value)
        assert lib.ddpm3d_conv3d_skip(C.byref(d), C.byref(sk), None) == H.E_INVAL, field
    d, sk = _pair(D=64, Hh=4, W=4, Cout=512, Cx=(512, 512))            # split 16 ways: needs its workspace
    d.workspace, d.workspace_bytes = 0, 0
    assert H.conv_plan(d)[2] > 1
    assert lib.ddpm3d_conv3d_skip(C.byref(d), C.byref(sk), None) == H.E_INVAL
    assert b"workspace" in lib.ddpm3d_last_error()
