"""
pack_ref.py without a GPU: the seeded inputs of test_gpu_pack.py satisfy the condition that makes a bit-exact
comparison fair (pack_ref.weights asserts it), the reference images have the sizes the library reports, and an
element sits where the layout's index formula says.
"""

import ctypes

import numpy as np
import pytest
import torch

import pack_ref as R
from guided_diffusion import _hip


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ddpm3d_packed_weight_bytes.restype = ctypes.c_size_t
    lib.ddpm3d_packed_up_phase_bytes.restype = ctypes.c_size_t
    return lib


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_seeded_inputs_keep_the_log2_margin_and_sizes_match(lib, case):
    Cout, Cin, k = case
    w = R.case_weights(*case)            # asserts the margin and the special couts' scales
    wz = "wz" in R.CASES[case][1]
    for precision in ((3, 4, 6) if wz else (0, 1, 2, 5)):
        assert R.image(w, precision).numel() == lib.ddpm3d_packed_weight_bytes(Cout, Cin, k, precision)
    if "up" in R.CASES[case][1]:
        assert sum(t.numel() for t in R.up_phase_image(w)) == lib.ddpm3d_packed_up_phase_bytes(Cout, Cin)


@pytest.mark.parametrize("precision", [0, 1, 5])
def test_an_element_sits_where_the_index_formula_says(precision):
    Cout, Cin, k = 40, 24, 3
    w = R.case_weights(Cout, Cin, k)
    CoutPad, CinPad = R.pads(Cout, Cin)
    img = R.image(w, precision).numpy()
    rng = np.random.default_rng(0)
    for _ in range(64):
        co, ci, tap = int(rng.integers(5, Cout)), int(rng.integers(Cin)), int(rng.integers(27))
        x = float(w.reshape(Cout, Cin, 27)[co, ci, tap])
        if precision == 0:
            at = ((tap * (CinPad // 8) + ci // 8) * CoutPad + co) * 8 + ci % 8
            assert img.view(np.float32)[at] == x
            continue
        body = 27 * CinPad * CoutPad * 4
        base = ((tap * (CinPad // 16) + ci // 16) * 2) * CoutPad * 16 + co * 16 + ci % 16
        wscale = float(img[body:].view(np.float32)[co])
        if precision == 5:
            bits = img[:body].view(np.int16)
            assert bits[base] == torch.tensor(x).bfloat16().view(torch.int16).item() and wscale == 1.0
            assert bits[base + CoutPad * 16] == 0
        else:
            half = img[:body].view(np.float16).astype(np.float64)
            hi, lo = half[base], half[base + CoutPad * 16]
            # hi + lo carries w * s to 2^-22 relative (two f16 roundings), 8 / 2 < max |w * s| <= 8
            assert abs((hi + lo) * wscale - x) <= 2.0 ** -21 * abs(x) + 2.0 ** -25 * wscale
