"""
The planner and its two replayers against tests/golden/plan_steps.json, recorded while engine.py still planned the
forward itself (tests/golden/make_plan_steps.py): per case the Python replay list has the recorded signature and
conv_meta, and the Python replay, the library's replay (native_plan) and the captured graph (step_graph) each give the
recorded bits of one forward and of three sampler steps.
"""

import json
import os

import pytest

import plan_steps as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_steps.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_step_list_and_bits_of_both_replayers_equal_the_recorded_ones(golden, name):
    case, g = P.CASES[name], golden[name]
    with P.switches(case):
        model, diff = P.build(case, "cuda")
        bits = {}
        for mode in ("python", "native", "graph"):
            model.native_plan, model.step_graph = mode == "native", mode == "graph"
            bits[mode] = P.outputs(model, diff, case)
        model.native_plan = model.step_graph = False
        eng = model.engine()
        plan = eng.plan(*P.ndhw(case.shape))
    assert eng.native_plans and any(pl.graphs for pl in eng.plans.values())      # both other replays really ran
    got = P.digest(P.signature(plan, eng.planar), P.meta(plan))
    assert got == {k: g[k] for k in got}
    for mode in ("python", "native", "graph"):
        assert bits[mode] == g["sha256"], mode
