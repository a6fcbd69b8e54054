#!/usr/bin/env python3
"""
Records tests/golden/conv_select.json: what the conv entries answer for the descriptor table of
tests/conv_select_cases.py -- return code and error text, kernel family, ddpm3d_conv_plan's three values and
ddpm3d_conv_skip_fused -- as one sha256 per block of cases plus a readable subset in full, one case per line.

Recorded at commit d907047 ("Plan the UNet forward in the library only; Python replays its steps"), i.e. while
conv_prepare, skip_prepare and the launchers still each decided their part of the kernel selection.  The queries need
no GPU (nothing is launched, no address is dereferenced), so the script runs on any tree whose library is built:

    python tests/golden/make_conv_select.py [out.json]
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "3d-denoising-diffusion-model_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_select_cases as S  # noqa: E402
from guided_diffusion import _hip as H  # noqa: E402


def main():
    blocks, shown = S.table(H.load())
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_select.json")
    with open(path, "w") as f:
        f.write('{\n"blocks": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in blocks.items()))
        f.write('\n},\n"cases": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in shown.items()))
        f.write("\n}\n}\n")
    print("%d cases in %d blocks, %d shown in full -> %s" % (sum(b["cases"] for b in blocks.values()), len(blocks),
                                                          len(shown), path))


if __name__ == "__main__":
    main()
