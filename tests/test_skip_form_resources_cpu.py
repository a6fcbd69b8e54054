"""
Host-side guard for the SKIP form of conv3d_wz_kernel.  The form stands at the register limit of two
workgroups per CU (256 VGPRs in the 4x4x8 tile form) and holds that only because its staging addresses are computed from
an opaque copy of the thread id and its scale / bias loads are deferred behind the tap loop; a compiler that hoists them
back spills.  A spill does not fail any arithmetic test, it only costs time, so the built library is asked directly: the
three SKIP instantiations, and the f16x3 forms they sit beside, report no scratch and at most 256 VGPRs in the code
object's own metadata (what -Rpass-analysis=kernel-resource-usage prints at build time).
"""

import os
import re
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_store_hazard as csh  # noqa: E402  (code_objects: the gfx950 code objects of libddpm3d.so)

READOBJ = os.path.join(csh.LLVM, "llvm-readobj")
LIB = os.path.join(ROOT, "3d-denoising-diffusion-model_amd", "csrc", "libddpm3d.so")


def _kernel_resources():
    """{mangled kernel name: (vgprs, scratch bytes, lds bytes)} over every code object of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in csh.code_objects(LIB, tmp):
            notes = subprocess.run([READOBJ, "--notes", f], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                g = {k: re.search(r"\.%s:\s*(\S+)" % k, blk) for k in
                     ("name", "vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
                if not all(g.values()):
                    continue
                out[g["name"].group(1).strip("'\"")] = (int(g["vgpr_count"].group(1)),
                                                        int(g["private_segment_fixed_size"].group(1)),
                                                        int(g["group_segment_fixed_size"].group(1)))
    return out


def test_skip_instantiations_have_no_scratch_and_two_workgroups_per_cu():
    if not os.path.exists(READOBJ):
        pytest.skip("no llvm-readobj here")
    res = _kernel_resources()
    # MODE 4 = WZ_F16X3_SKIP, 0 = WZ_F16X3, 3 = WZ_F16X3_UP (conv3d_stage.h); IL 4; tile forms 8x8x2, 8x4x4, 4x4x8
    # (the Itanium names of conv3d_wz_kernel<MODE, IL, TX, TY>(ConvK))
    want = ["_Z16conv3d_wz_kernelILi%dELi4ELi%dELi%dEEv5ConvK" % (m, tx, ty) for m in (4, 0, 3)
            for tx, ty in ((8, 8), (8, 4), (4, 4))]
    for w in want:
        hit = [(n, r) for n, r in res.items() if n == w]
        assert len(hit) == 1, (w, [n for n, _ in hit], sorted(n for n in res if "conv3d_wz_kernel" in n))
        vgprs, scratch, _ = hit[0][1]
        print(hit[0][0], "VGPRs", vgprs, "scratch", scratch)
        # 512 registers per lane of a SIMD, two waves: 256 is the most a wave may hold with two workgroups of four
        # waves on a CU's four SIMDs
        assert scratch == 0 and vgprs <= 256, hit[0]
