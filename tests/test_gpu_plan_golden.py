"""GPU: the batch planner's decisions are pinned.  For every case of tests/golden/make_plan_golden.py -- TDNN with statistics
and attentive pooling, extended TDNN, ResNet-18; precisions, nodes, ragged and uniform batches, every planner option on and
off -- the xv_plan_info fields (output shape, workspace_bytes = the top of the workspace arena, flops) and the steps of one
profiled forward (name, launches, flops, bytes, in order) must EQUAL tests/golden/plan_info.json, which was recorded with
the same recorder on a build of the commit before the planner was split into phases.  Step order, every fusion decision
and the arena layout are fixed by these numbers; a deliberate change of a plan re-records the file on the parent build.
One decision is NOT visible here: `grid_compact` 0 / 1 (compact or full enumeration of a grid convolution's rows) changes
only the row maps, which live outside the workspace, and neither a step's flops nor its bytes -- those cases equal their
default twins.  That choice is held by test_gpu_variants.test_compact_grid_rows_are_bit_identical_to_the_full_enumeration."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_plan_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_plan_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

GROUPS = ["tdnn_stat/f32", "tdnn_stat/bf16x3", "tdnn_stat/f16f6",
          "tdnn_att_h1/bf16x3", "tdnn_att_h1/f32", "tdnn_att_h3/bf16x3", "tdnn_att_h3/f32", "tdnn_att_h5/bf16x3", "tdnn_att_h5/f32",
          "etdnn/f16f6", "etdnn/f16x3",
          "resnet_plain/f32", "resnet_plain/bf16x3", "resnet_plain/f16f6",
          "resnet_ts_max/f32", "resnet_ts_max/bf16x3", "resnet_ts_max/f16f6"]


@pytest.fixture(scope="module")
def golden():
    return recorder.load_golden()


def test_the_case_list_is_the_recorded_one(golden):
    specs = dict(recorder.groups())
    assert list(specs) == GROUPS
    want = {"%s/%s/%s/%s" % (gid, recorder._key(dict(pre, **opts)), batch, node)
            for gid, spec in specs.items() for pre, plans in spec["runs"] for opts, batch, node in plans}
    assert want == set(golden)


@pytest.mark.parametrize("gid", GROUPS)
def test_plans_equal_the_recorded_ones(gid, golden):
    got = recorder.run_group(dict(recorder.groups())[gid])
    assert got, gid
    for key, rec in got.items():
        want = golden["%s/%s" % (gid, key)]
        assert rec["info"] == want["info"], (gid, key)
        assert rec["steps"] == want["steps"], (gid, key)
