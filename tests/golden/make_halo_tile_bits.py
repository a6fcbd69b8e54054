#!/usr/bin/env python3
"""
Record tests/golden/halo_tile_bits.json on an MI355X: the SHA-256 of every D plane of ddpm3d_sphere_mean's and
ddpm3d_nlm's output for the 25 centred cases of tests/halo_tile_cases.py, from a trusted build of the library:

    DDPM3D_LIB=<that build's libddpm3d.so> python tests/golden/make_halo_tile_bits.py COMMIT [OUT.json]

COMMIT is the id of the commit the library was built from; it and the compiler's version line are stored beside the
digests.  The inputs come from the yardsticks' seeded numpy generators.  Non-local means calls expf, so the bits belong
to the toolchain as well as to the source: after a compiler change, record again from the commit before that change.
"""

import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.dont_write_bytecode = True
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "3d-denoising-diffusion-model_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import baseline_ref as B  # noqa: E402
import halo_tile_cases as C  # noqa: E402
from guided_diffusion import metrics  # noqa: E402


def main():
    if len(sys.argv) not in (2, 3) or not os.environ.get("DDPM3D_LIB"):
        sys.exit("usage: DDPM3D_LIB=<the trusted build> python tests/golden/make_halo_tile_bits.py COMMIT [OUT.json]")
    if not torch.cuda.is_available():
        sys.exit("make_halo_tile_bits: needs a GPU")
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    cases = {}
    for keep, radii, _, _ in C.PEAK_CLASSES:
        x, mask, half_w, _ = C.peak_case(keep, radii, 0.0)
        fp = metrics.SphereFootprint(None, None, None, radii, half_w)
        out = metrics.sphere_mean(dev(x), fp, keep=None if mask is None else dev(mask))
        cases[C.peak_key(keep, radii)] = C.plane_digests(out.cpu().numpy())
    for search, patch, _, _, _ in C.NLM_CLASSES:
        x, h = B.nlm_case(C.SHAPE, search, patch, 0.0)[:2]
        out = metrics.nlm(dev(x), h, search=search, patch=patch)
        cases[C.nlm_key(search, patch)] = C.plane_digests(out.cpu().numpy())
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    version = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()
    version = "; ".join(line.strip() for line in version[:2])
    record = {"what": "SHA-256 of every D plane of the outputs of tests/halo_tile_cases.py's centred cases on an MI355X",
              "commit": sys.argv[1], "hipcc": version, "shape": list(C.SHAPE),
              "cases": cases}
    path = sys.argv[2] if len(sys.argv) == 3 else os.path.join(HERE, "halo_tile_bits.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote %s: %d cases" % (path, len(cases)))


if __name__ == "__main__":
    main()
