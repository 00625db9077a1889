"""fpcc_conv_f32_plan is the one classification of a convolution shape; the six older shape queries read it.  The table under
tests/golden was recorded (tools/dump_conv_plan_table.py) with the library of the commit before the plan existed: no answer moved.
The library loads without a GPU."""
import ctypes
import itertools
import json
import os
import sys

import pytest

from fastpcc_amd import hipops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import dump_conv_plan_table as dump  # noqa: E402


@pytest.fixture(scope='module')
def parent():
    with open(os.path.join(ROOT, 'tests', 'golden', 'conv_plan_parent.json')) as f:
        doc = json.load(f)
    points = list(itertools.product(*doc['axes'].values()))
    assert list(doc['axes']) == ['c1', 'c2', 'c_out', 'n_offsets', 'groups'] and len(points) == 8 * 4 * 7 * 6 * 3
    assert all(len(col) == len(points) for col in doc['columns'].values())
    return points, doc['columns']


def test_grid_has_the_edges_of_every_rule(parent):
    points, cols = parent
    axes = [set(p[i] for p in points) for i in range(5)]
    assert axes[0] >= {1, 16, 32, 48, 64, 256, 512, 544} and axes[1] >= {0, 16, 32, 256}
    assert axes[2] >= {1, 8, 32, 64, 128, 255, 256} and axes[3] >= {1, 7, 8, 27, 28, 32} and axes[4] >= {1, 2, 8}
    assert set(cols['order_ex']) == {0, 1, 3} and set(cols['natural_matrix']) == {0, 1}        # every family occurs
    assert any(cols['packed_floats']) and any(cols['packed_floats_nat']) and any(cols['ws_bytes_5'])


def test_old_queries_answer_as_before_the_plan(parent):
    points, cols = parent
    lib = hipops.lib()
    for i, point in enumerate(points):
        got = dump.answers(lib, *point)
        assert set(got) == set(cols)
        assert got == {name: col[i] for name, col in cols.items()}, point


def test_plan_fields_are_the_old_answers(parent):
    points, cols = parent
    lib = hipops.lib()
    index = {point: i for i, point in enumerate(points)}
    for i, point in enumerate(points):
        p = hipops.ConvPlan()
        assert lib.fpcc_conv_f32_plan(*point, ctypes.byref(p)) == 0
        old = dump.answers(lib, *point)
        assert p.order == old['order_ex'], point
        assert p.matrix == int(old['order_ex'] != 0 or old['natural_matrix'] != 0), point
        assert not (old['packed_floats'] and old['packed_floats_nat']), point
        assert p.packed == (1 if old['packed_floats'] else 2 if old['packed_floats_nat'] else 0), point
        assert p.packed_floats == old['packed_floats'] + old['packed_floats_nat'], point
        assert p.ws_bytes == old['ws_bytes_5'] and old['ws_bytes_0'] == 0, point
        # chunk is a property of (c1, c2, c_out): 32 where the one-offset, one-group shape has an order-1 image, else 16 where it has an
        # MFMA order, else 0
        one = index[point[:3] + (1, 1)]
        assert p.chunk == (32 if cols['packed_floats'][one] else 16 if cols['order'][one] else 0), point
        if 1 <= point[3] <= 27:
            assert (p.chunk == 32) == (old['packed_floats'] != 0), point
        q = hipops.conv_plan(*point)
        assert [getattr(q, f) for f, _ in p._fields_] == [getattr(p, f) for f, _ in p._fields_], point
        assert hipops.conv_order(*point) == p.order and hipops.conv_order(*point, 12345) == p.order
        assert hipops.conv_natural_matrix(*point) == bool(old['natural_matrix'])


def test_plan_refuses_a_null_pointer():
    assert hipops.lib().fpcc_conv_f32_plan(32, 0, 32, 1, 1, None) != 0
    assert b'conv_f32_plan' in hipops.lib().fpcc_last_error()


def test_set_tuning_clears_the_cached_plans():
    hipops.conv_plan(32, 0, 32, 27, 1)
    assert hipops.conv_plan.cache_info().currsize > 0
    before = hipops.conv_set_tuning(hipops.KNOB_WAVE_SB, 0)                 # result-neutral
    try:
        assert hipops.conv_plan.cache_info().currsize == 0
    finally:
        hipops.conv_set_tuning(hipops.KNOB_WAVE_SB, before)
    assert hipops.conv_plan.cache_info().currsize == 0
