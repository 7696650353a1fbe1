"""CPU-side checks of step_03 --debug_mode: output names, routing, C-ABI bookkeeping and tools/compare_deltas.py.
No compute call is made here; the kernels and the file functions are checked in tests/test_step03_debug_hip.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'compare_deltas.py')


def test_output_names_of_both_modes():
    """step_03:355-357 and :405-407: beside the output path, `{var_name_map[v]}_delta_{name}` and `delta_{v}_{name}`."""
    from pgw4era5_amd import step_03_debug as dbg
    out = os.path.join('some', 'dir', 'cas20060802030000.nc')
    want = dict(ps='PS', ta='T', hur='RELHUM', ua='U', va='V', st='T_SO', ts='T_SKIN')
    assert dbg.FULL_VARS == ('ps', 'ta', 'hur', 'ua', 'va', 'st', 'ts')
    for v in dbg.FULL_VARS:
        assert dbg.full_delta_path(out, v) == os.path.join('some', 'dir', '%s_delta_cas20060802030000.nc' % want[v])
    assert dbg.TIME_VARS == ('tos', 'tas', 'hurs', 'ps', 'ta', 'hur', 'ua', 'va', 'zg')
    for v in dbg.TIME_VARS:
        assert dbg.time_delta_path(out, v) == os.path.join('some', 'dir', 'delta_%s_cas20060802030000.nc' % v)


def test_debug_functions_are_never_pipelined():
    """parallel.run_shard pipelines a function that has `stages`; the debug functions have none, and the stages of
    pgw_for_era5 still refuse a debug mode."""
    from pgw4era5_amd import step_03_debug as dbg, step_03_apply_to_era as s3
    assert not hasattr(dbg.debug_interpolate_full, 'stages') and not hasattr(dbg.debug_interpolate_time, 'stages')
    with pytest.raises(NotImplementedError):
        s3._stage_load('a.nc', 'b.nc', 'd', None, True, debug_mode='interpolate_full')


@pytest.mark.parametrize('mode', ['interpolate_time', 'interpolate_full'])
def test_bands_with_debug_mode_is_still_refused(tmp_path, mode):
    from pgw4era5_amd import step_03_apply_to_era as s3
    with pytest.raises(NotImplementedError):
        s3._cli(['-i', str(tmp_path), '-o', str(tmp_path / 'out'), '-d', str(tmp_path), '-f', '2006080200', '-l', '2006080200',
                 '--bands', '-D', mode])


def test_new_entries_are_declared_bound_and_have_a_kernel_id():
    from pgw4era5_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    for name in ('pgw_delta_fields', 'pgw_surface_deltas'):
        assert name in _lib.SIGNATURES and name + '(' in hdr
    assert 'PGW_K_DELTA_FIELDS = %d' % _lib.KERNEL_IDS['delta_fields'] in hdr
    assert 'PGW_K_COUNT = %d' % len(_lib.KERNEL_IDS) in hdr
    assert len(_lib.SIGNATURES['pgw_delta_fields'][1]) == 30
    assert len(_lib.SIGNATURES['pgw_surface_deltas'][1]) == 24


def _write_dir(path, arrays):
    from pgw4era5_amd import ncio
    os.makedirs(path, exist_ok=True)
    for fname, (var, values) in arrays.items():
        ds = ncio.Dataset()
        dims = ('time', 'level', 'lat', 'lon') if values.ndim == 4 else ('time', 'lat', 'lon')
        ds['time'] = ncio.Field(np.array([0.0]), ('time',))
        ds[var] = ncio.Field(values, dims)
        ncio.to_netcdf(ds, os.path.join(path, fname))


def _run_tool(*args):
    r = subprocess.run([sys.executable, TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    return r, line


def test_compare_deltas_tool(tmp_path):
    rng = np.random.default_rng(0)
    t = rng.standard_normal((1, 3, 4, 5))
    ts = rng.standard_normal((1, 4, 5)).astype(np.float32)
    ts[0, 1, 2] = np.nan
    base = {'T_delta_cas.nc': ('T', t), 'T_SKIN_delta_cas.nc': ('T_SKIN', ts)}
    _write_dir(tmp_path / 'a', base)
    _write_dir(tmp_path / 'b', base)
    r, line = _run_tool(tmp_path / 'a', tmp_path / 'b')
    assert r.returncode == 0, r.stdout + r.stderr
    assert line['ok'] is True and line['compared'] == 2 and line['failed'] == []
    assert line['files']['T_delta_cas.nc']['max_abs'] == 0.0 and line['files']['T_SKIN_delta_cas.nc']['nan_mask_equal'] is True
    assert line['files']['T_SKIN_delta_cas.nc']['dtype_a'] == 'float32' and line['files']['T_delta_cas.nc']['dtype_b'] == 'float64'
    # one perturbed value: non-zero exit, the file named, the figure reported; within --atol it passes again
    t2 = t.copy()
    t2[0, 1, 2, 3] += 1e-3
    _write_dir(tmp_path / 'c', {'T_delta_cas.nc': ('T', t2), 'T_SKIN_delta_cas.nc': ('T_SKIN', ts)})
    r, line = _run_tool(tmp_path / 'a', tmp_path / 'c')
    assert r.returncode != 0 and line['failed'] == ['T_delta_cas.nc']
    assert 'T_delta_cas.nc' in r.stdout and 'DIFFERS' in r.stdout
    assert abs(line['files']['T_delta_cas.nc']['max_abs'] - 1e-3) < 1e-12
    r, line = _run_tool(tmp_path / 'a', tmp_path / 'c', '--atol', '2e-3')
    assert r.returncode == 0 and line['ok'] is True
    # differing NaN masks are reported and fail whatever the tolerance
    ts2 = ts.copy()
    ts2[0, 0, 0] = np.nan
    _write_dir(tmp_path / 'd', {'T_delta_cas.nc': ('T', t), 'T_SKIN_delta_cas.nc': ('T_SKIN', ts2)})
    r, line = _run_tool(tmp_path / 'a', tmp_path / 'd', '--atol', '1.0')
    assert r.returncode != 0 and line['failed'] == ['T_SKIN_delta_cas.nc']
    assert line['files']['T_SKIN_delta_cas.nc']['nan_mask_equal'] is False and line['files']['T_SKIN_delta_cas.nc']['why'] == 'nan mask'
    # nothing in common is not a pass; files of one side only are listed
    _write_dir(tmp_path / 'e', {'U_delta_cas.nc': ('U', t)})
    r, line = _run_tool(tmp_path / 'a', tmp_path / 'e')
    assert r.returncode != 0 and line['compared'] == 0 and line['only_b'] == ['U_delta_cas.nc']
