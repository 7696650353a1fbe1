"""Host-side checks of the two fields that carry zg's own plev axis through the C-ABI (pgw_file_args.nplev_zg / plev_zg):
the ctypes mirror against the header as a C compiler lays it out, and the file plan around it.  No GPU, no library."""
import ctypes as C
import os
import re
import subprocess

from pgw4era5_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'pgw_hip.h')


def test_file_args_end_with_the_zg_axis():
    names = [f[0] for f in _lib.FileArgs._fields_]
    assert names[-3:] == ['nplev_zg', '_pad1', 'plev_zg']
    assert names[-4] == 'tos_x_new'                                  # appended: everything before keeps its place
    assert _lib.FileArgs.nplev_zg.offset == _lib.FileArgs.tos_x_new.offset + 8
    assert _lib.FileArgs.plev_zg.offset == _lib.FileArgs.nplev_zg.offset + 8
    assert C.sizeof(_lib.FileArgs) == _lib.FileArgs.plev_zg.offset + 8
    a = _lib.FileArgs()
    assert a.nplev_zg == 0 and not a.plev_zg                        # the default: zg shares plev


def test_file_args_layout_is_the_c_compiler_s(tmp_path):
    """sizeof and the offsets of a few members, first, middle and last, as `cc` sees include/pgw_hip.h."""
    members = ('dtype', 'ncol', 'plev', 'zg3_b', 'x_hi', 'PS_out', 'n_iter', 'max_err_hist', 'per_var_time', 'zg_x_hi',
               'tos_x_new', 'nplev_zg', 'plev_zg')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pgw_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(pgw_file_args), sizeof(pgw_file_plan));\n' +
                   ''.join('  printf("%%zu\\n", offsetof(pgw_file_args, %s));\n' % m for m in members) +
                   '  printf("%zu\\n", offsetof(pgw_file_plan, n_axes));\n  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call([os.environ.get('CC', 'cc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert int(out[0]) == C.sizeof(_lib.FileArgs) and int(out[1]) == C.sizeof(_lib.FilePlan)
    for m, off in zip(members, out[2:]):
        assert int(off) == getattr(_lib.FileArgs, m).offset, m
    assert int(out[-1]) == _lib.FilePlan.n_axes.offset


def test_plan_offsets_keep_their_relations():
    """The relations tests/test_delta_bracket_host.py pins: the plan's members follow the argument struct."""
    assert _lib.FilePlan.args.offset == 0 and _lib.FilePlan.n_axes.offset == C.sizeof(_lib.FileArgs)
    assert C.sizeof(_lib.PlanVar) == 32
    assert C.sizeof(_lib.FilePlan) == C.sizeof(_lib.FileArgs) + 8 + 8 * 8 + 4 * 8 + 32 * 11


def test_limits_match_the_header():
    txt = open(HEADER).read()
    assert int(re.search(r'#define PGW_MAX_PLEV (\d+)', txt).group(1)) == _lib.MAX_PLEV == 128
    assert int(re.search(r'#define PGW_MAX_PLEV_ZG (\d+)', txt).group(1)) == _lib.MAX_PLEV_ZG == 64
    assert '[2, 64]' not in txt and '2 <= nplev <= 128' in txt
