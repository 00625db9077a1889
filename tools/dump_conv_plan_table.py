"""Records what the six shape queries of libfpcc_hip.so answer on a grid of convolution shapes (no GPU needed):

    python tools/dump_conv_plan_table.py tests/golden/conv_plan_parent.json

tests/golden/conv_plan_parent.json was written by this script with the library of the commit BEFORE fpcc_conv_f32_plan existed;
tests/test_conv_plan.py holds every later library to it.  One list per query, in itertools.product order of the axes."""
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AXES = {'c1': [1, 16, 32, 48, 64, 256, 512, 544], 'c2': [0, 16, 32, 256], 'c_out': [1, 8, 32, 64, 128, 255, 256],
        'n_offsets': [1, 7, 8, 27, 28, 32], 'groups': [1, 2, 8]}


def answers(lib, c1, c2, c_out, n_offsets, groups):
    """the six old queries at one grid point, the workspace query at n_out = 0 and n_out = 5"""
    shape = (c1, c2, c_out, n_offsets, groups)
    return {'order': lib.fpcc_conv_f32_order(c1, c2, c_out),
            'order_ex': lib.fpcc_conv_f32_order_ex(*shape, 5),
            'natural_matrix': lib.fpcc_conv_f32_natural_matrix(*shape),
            'ws_bytes_0': lib.fpcc_conv_f32_ws_bytes(*shape, 0),
            'ws_bytes_5': lib.fpcc_conv_f32_ws_bytes(*shape, 5),
            'packed_floats': lib.fpcc_conv_packed_floats(*shape),
            'packed_floats_nat': lib.fpcc_conv_packed_floats_nat(*shape)}


def table(lib):
    cols = {}
    for point in itertools.product(*AXES.values()):
        for name, value in answers(lib, *point).items():
            cols.setdefault(name, []).append(int(value))
    return cols


if __name__ == '__main__':
    from fastpcc_amd import hipops
    doc = {'axes': AXES, 'columns': table(hipops.lib())}
    with open(sys.argv[1], 'w') as f:
        f.write('{"axes": ' + json.dumps(AXES) + ',\n "columns": {\n' +
                ',\n'.join(f'  "{k}": ' + json.dumps(v, separators=(',', ':')) for k, v in doc['columns'].items()) + '\n }}\n')
