"""
What the nine step entries (ddpm3d_{p_sample,ddim,dpm_solver}_step{,_keyed,_x0}) and the two q_sample entries refuse,
precedence included: from a valid call of each entry, every single fault of a list and every pair of them, and the
(return code, ddpm3d_last_error() text) of each compared with tests/golden/step_entry_errors.json, which was recorded on
a host without a GPU from a build of the commit its header names:

    DDPM3D_LIB=<that build's libddpm3d.so> python tests/test_step_entries_cpu.py --record COMMIT

Every address is a fake non-null 16-byte aligned number; nothing is ever dereferenced, because every case carries at
least one fault and so fails validation before any HIP call: the code is never DDPM3D_OK and never E_LAUNCH.  The test
is skipped where a GPU is visible: a regression that dropped a check must fail here, where a launch has no device to
reach, and must never launch on fake addresses on a shared machine.

A fault is applied to the entries whose contract (include/ddpm3d.h) refuses it, and to no other: the list below says
which.  The two oldest entries, ddpm3d_p_sample_step and ddpm3d_ddim_step, and their keyed forms document no refusal
of unknown flag bits or of aliased tensors, and pred_xstart may be NULL there; the un-keyed two take any N > 0 (the
launch itself refuses a grid beyond 65535 rows).  For the solver a NULL noise or key is the ODE form and a NULL
x0_prev* is a fault only at the order that reads it.  Only the x0 entries take both a noise tensor and a key, and only
they refuse outputs that alias what the call reads.
"""

import itertools
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN
from guided_diffusion import _hip

GOLDEN_FILE = os.path.join(GOLDEN, "step_entry_errors.json")
F = 1 << 20             # fake addresses are multiples of it
ADDR = dict(model_out=1, xstart=2, x=3, noise=4, coef=5, t_idx=6, sample=7, x0_prev1=8, x0_prev2=9, scoef=10,
            pred_xstart=11, key_stream=12, key_origin=13, x_start=3, qcoef=5, x_t=7)
GOOD_KEY = dict(seed=1, stream=ADDR["key_stream"] * F, draw=1, origin=None, patch=(0, 0, 0), canvas=(0, 0, 0))
KINDS = {"p_sample": "ddpm", "ddim": "ddim", "dpm_solver": "solver"}


def entries():
    """{entry name: (kind, style, the ordered valid arguments)}; a key is a dict until the call"""
    e = {}
    for stem, kind in KINDS.items():
        solver = kind == "solver"
        for style, suffix in (("plain", ""), ("keyed", "_keyed"), ("x0", "_x0")):
            names = ["model_out"] + ["xstart"] * (style == "x0") + ["x"] + ["x0_prev1", "x0_prev2"] * solver
            names += {"plain": ["noise"], "keyed": ["key"], "x0": ["noise", "key"]}[style]
            names += ["coef"] + ["scoef"] * solver + ["t_idx", "N", "voxels"] + ["T"] * solver + ["flags"]
            names += ["eta"] * (kind == "ddim") + ["order"] * solver + ["sample", "pred_xstart", "stream"]
            e["ddpm3d_%s_step%s" % (stem, suffix)] = (kind, style, names)
    e["ddpm3d_q_sample"] = ("q", "plain", ["x_start", "noise", "qcoef", "t_idx", "N", "voxels", "T", "x_t", "stream"])
    e["ddpm3d_q_sample_keyed"] = ("q", "keyed", ["x_start", "key", "qcoef", "t_idx", "N", "voxels", "T", "x_t", "stream"])
    scalars = dict(N=2, voxels=64, T=10, flags=_hip.F_LEARN_SIGMA, eta=0.5, order=3, stream=None)
    out = {}
    for name, (kind, style, names) in e.items():
        a = {n: scalars[n] if n in scalars else ADDR[n] * F for n in names if n != "key"}
        if "key" in names:
            a["key"] = dict(GOOD_KEY) if style == "keyed" else None
        out[name] = (kind, style, {n: a[n] for n in names})
    return out


ENTRIES = entries()


def keyed(a, **over):
    """the call reads its noise from a key with `over`: the x0 entries drop their noise tensor for it"""
    a["key"] = dict(a["key"] or GOOD_KEY, **over)
    if "noise" in a:
        a["noise"] = None


def geometry(a, **over):
    keyed(a, **dict(dict(origin=ADDR["key_origin"] * F, patch=(4, 4, 4), canvas=(8, 8, 8)), **over))


def faults(kind, style, args):
    """[(name, mutation of the argument dict)] in the order pairs apply them, for one entry"""
    solver, x0, has_key = kind == "solver", style == "x0", "key" in args
    optional = {"stream"}
    if kind in ("ddpm", "ddim") and not x0:
        optional.add("pred_xstart")                      # "pred_xstart may be NULL"
    if x0:
        optional.add("key")                              # one of noise and key: the faults "neither" and "both"
        if kind != "ddpm":
            optional.add("model_out")                    # read by p_sample_step_x0 under F_LEARN_SIGMA only
        if not solver:
            optional.add("pred_xstart")
    if solver:
        optional |= {"noise", "key", "x0_prev1", "x0_prev2"}         # the ODE form; the history has faults of its own
    f = []
    for n, v in args.items():
        if (isinstance(v, int) and v >= F or n == "key" and v is not None) and n not in optional:
            f.append(("null:" + n, lambda a, n=n: a.__setitem__(n, None)))
    f.append(("N=0", lambda a: a.update(N=0)))
    if not (kind in ("ddpm", "ddim") and style == "plain"):
        f.append(("N=65536", lambda a: a.update(N=65536)))
    f.append(("voxels=0", lambda a: a.update(voxels=0)))
    if "T" in args:
        f.append(("T=0", lambda a: a.update(T=0)))
    if "flags" in args and (solver or x0):
        f.append(("flags=8", lambda a: a.update(flags=8)))
    if solver:
        f.append(("order=0", lambda a: a.update(order=0)))
        f.append(("order=4", lambda a: a.update(order=4)))
        f.append(("order=2,no_prev1", lambda a: a.update(order=2, x0_prev1=None)))
        f.append(("order=3,no_prev2", lambda a: a.update(order=3, x0_prev2=None)))
    if has_key:
        f.append(("key.stream=NULL", lambda a: keyed(a, stream=None)))
        f.append(("key.draw=-1", lambda a: keyed(a, draw=-1)))
        f.append(("patch!=voxels", lambda a: geometry(a, patch=(4, 4, 5))))
        f.append(("canvas=0", lambda a: geometry(a, canvas=(8, 0, 8))))
    if x0:
        f.append(("both", lambda a: a.update(noise=ADDR["noise"] * F, key=a["key"] or dict(GOOD_KEY))))
        if not solver:
            f.append(("neither", lambda a: a.update(noise=None, key=None)))
        inputs = ["model_out", "xstart", "x", "noise"] + ["x0_prev1", "x0_prev2"] * solver
        for o in ("sample", "pred_xstart"):
            for i in inputs:
                f.append(("%s=%s" % (o, i), lambda a, o=o, i=i: a.__setitem__(o, ADDR[i] * F)))
        f.append(("sample=pred_xstart", lambda a: a.update(sample=ADDR["pred_xstart"] * F,
                                                           pred_xstart=ADDR["pred_xstart"] * F)))
    return f


def call(lib, entry, args):
    a = dict(args)
    if a.get("key") is not None:
        k = _hip.NoiseKeyDesc()
        k.seed, k.stream, k.draw, k.origin = a["key"]["seed"], a["key"]["stream"], a["key"]["draw"], a["key"]["origin"]
        k.patch[:], k.canvas[:] = a["key"]["patch"], a["key"]["canvas"]
        a["key"] = k
    rc = getattr(lib, entry)(*a.values())
    return [rc, lib.ddpm3d_last_error().decode()]


def results(entry):
    """{case name: [code, message]} of every single fault and every pair, the pair's faults applied in list order"""
    lib = _hip.load()
    kind, style, base = ENTRIES[entry]
    fl = faults(kind, style, base)
    out = {}
    for combo in [(f,) for f in fl] + list(itertools.combinations(fl, 2)):
        a = {n: dict(v) if isinstance(v, dict) else v for n, v in base.items()}
        for _, mutate in combo:
            mutate(a)
        out[" + ".join(n for n, _ in combo)] = call(lib, entry, a)
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_FILE) as f:
        g = json.load(f)
    return {e: {case: g["results"][i] for case, i in cases.items()} for e, cases in g["entries"].items()}


def test_every_entry_is_covered(recorded):
    assert sorted(recorded) == sorted(ENTRIES) and len(ENTRIES) == 11


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake addresses must never reach a device")
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_are_the_recorded_ones(recorded, entry):
    got = results(entry)
    assert sorted(got) == sorted(recorded[entry])
    passed = [c for c, (rc, _) in got.items() if rc in (0, _hip.E_LAUNCH)]
    assert not passed, "passed validation: %s" % passed[:5]
    differ = {c: (got[c], recorded[entry][c]) for c in got if got[c] != recorded[entry][c]}
    assert not differ, "%d of %d differ, e.g. %s" % (len(differ), len(got), list(differ.items())[:3])


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: DDPM3D_LIB=<the trusted build> python tests/test_step_entries_cpu.py --record COMMIT")
    assert not torch.cuda.is_available(), "record on a host without a GPU"
    table, entries_out = [], {}
    for entry in sorted(ENTRIES):
        entries_out[entry] = {}
        for case, res in results(entry).items():
            assert res[0] not in (0, _hip.E_LAUNCH), (entry, case, res)
            if res not in table:
                table.append(res)
            entries_out[entry][case] = table.index(res)
    header = "[code, ddpm3d_last_error()] per entry and case (an index into results); recorded on a host without a " \
             "GPU from a build of commit %s" % sys.argv[2]
    with open(GOLDEN_FILE, "w") as f:
        json.dump({"header": header, "results": table, "entries": entries_out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d distinct results" % (GOLDEN_FILE, sum(len(v) for v in entries_out.values()),
                                                       len(table)))
