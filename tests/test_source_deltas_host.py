"""settings.delta_grid = 'source' without a GPU: the flag on the argument surface, the three regrid-plan entries in header,
binding and library, the errors that must come before any library call (on the recording stand-in of
tests/function_recorder.py), and the conditions the cases of tests/source_delta_cases.py exist for."""
import os
import re

import numpy as np
import pytest

import source_delta_cases as K
from function_recorder import RecordingContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('pgw_regrid_plan_create', 'pgw_regrid_plan_apply', 'pgw_regrid_plan_destroy')


@pytest.fixture
def clean_mode(monkeypatch):
    """PGW_DELTA_GRID as the test found it afterwards (the command line sets it for the ranks it starts)."""
    monkeypatch.setenv('PGW_DELTA_GRID', 'era5')                    # registered, so that whatever a test leaves is undone
    monkeypatch.delenv('PGW_DELTA_GRID')
    return monkeypatch


def test_case_conditions():
    assert K.conditions()


def test_the_three_entries_are_declared_bound_and_exported():
    from pgw4era5_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and re.search(r'\bint %s\(' % name, hdr), name
    i, ll, vp, ip, dp = _lib._i, _lib._ll, _lib._vp, _lib._ip, _lib._dp
    tables = [ip, ip, dp, dp, ip]                                   # lo, hi, dx, Dx, oob of one axis: pgw_regrid_bilinear's order
    assert _lib.SIGNATURES['pgw_regrid_plan_create'] == (i, [vp, i, i, i, i] + tables + tables + [i, i, ll, _lib._vpp])
    assert _lib.SIGNATURES['pgw_regrid_bilinear'][1][8:18] == tables + tables
    assert _lib.SIGNATURES['pgw_regrid_plan_apply'] == (i, [vp, vp, i, i, ll, vp, vp])
    assert _lib.SIGNATURES['pgw_regrid_plan_destroy'] == (i, [vp, vp])
    assert 'PGW_K_COUNT = 28' in hdr and _lib.KERNEL_IDS['regrid'] == 8 and len(_lib.KERNEL_IDS) == 28
    assert os.path.exists(_lib.LIB_PATH), 'libpgw_hip.so is not built'
    blob = open(_lib.LIB_PATH, 'rb').read()
    for name in ENTRIES:
        assert name.encode() + b'\0' in blob, '%s is not in the library' % name


def test_flag_and_setting_on_the_argument_surface(clean_mode, tmp_path, capsys):
    from pgw4era5_amd import settings as S, step_03_apply_to_era as s3
    assert S.delta_grid == 'era5' and s3.delta_grid_mode() == 'era5'
    with pytest.raises(SystemExit):
        s3._cli(['--help'])
    assert '--delta_grid {era5,source}' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        s3._cli(['-i', 'a', '-o', 'b', '-d', 'c', '--delta_grid', 'gcm'])
    # the flag reaches the ranks of -p N through the environment they inherit, and is checked before anything is made
    out = tmp_path / 'out'
    with pytest.raises(ValueError, match='--bands'):
        s3._cli(['-i', str(tmp_path), '-o', str(out), '-d', str(tmp_path), '--delta_grid', 'source', '--bands'])
    assert 'PGW_DELTA_GRID' not in os.environ and not out.exists()  # set for the ranks while the command runs, then put back
    seen = []
    clean_mode.setattr(s3, '_run_cli', lambda args: seen.append(os.environ.get('PGW_DELTA_GRID')))
    s3._cli(['-i', 'a', '-o', str(out), '-d', 'c', '--delta_grid', 'source', '-p', '2'])
    clean_mode.setenv('PGW_DELTA_GRID', 'source')
    s3._cli(['-i', 'a', '-o', str(out), '-d', 'c', '--delta_grid', 'era5'])
    s3._cli(['-i', 'a', '-o', str(out), '-d', 'c'])
    assert seen == ['source', 'era5', 'source'] and os.environ['PGW_DELTA_GRID'] == 'source' and not out.exists()
    assert s3.delta_grid_mode() == 'source'
    clean_mode.setenv('PGW_DELTA_GRID', 'era5')
    clean_mode.setattr(S, 'delta_grid', 'source')
    assert s3.delta_grid_mode() == 'era5'                          # the environment overrides the setting
    clean_mode.delenv('PGW_DELTA_GRID')
    assert s3.delta_grid_mode() == 'source'


def _era5(lat, lon, two_d=False):
    from pgw4era5_amd import ncio
    ds = ncio.Dataset()
    if two_d:
        la, lo = np.meshgrid(lat, lon, indexing='ij')
        ds['lat'] = ncio.Field(la, ('rlat', 'rlon'))
        ds['lon'] = ncio.Field(lo, ('rlat', 'rlon'))
    else:
        ds['lat'] = ncio.Field(np.asarray(lat, dtype=np.float64), ('lat',))
        ds['lon'] = ncio.Field(np.asarray(lon, dtype=np.float64), ('lon',))
    ds['FR_LAND'] = ncio.Field(np.zeros((1, len(lat), len(lon))), ('time', 'lat', 'lon') if not two_d else ('time', 'rlat', 'rlon'))
    return ds


def test_errors_come_before_any_library_call(clean_mode, tmp_path):
    """bands, the xESMF setting, a bad value, an ERA5 file with 2-D lat / lon, a source that does not cover the target (the
    reference's message): ValueError with no pgw_* call recorded and nothing uploaded."""
    from pgw4era5_amd import settings as S, step_03_apply_to_era as s3, synthetic
    ctx = RecordingContext()
    ctx.device = 0
    gcm = str(tmp_path / 'gcm')
    synthetic.write_gcm_files(gcm, nlat=5, nlon=8, plev=[100000.0, 50000.0, 10000.0], ocean=(6, 8))
    inside = _era5([-40.0, 0.0, 40.0], [10.0, 20.0, 30.0])
    clean_mode.setattr(S, 'delta_grid', 'source')
    clean_mode.setattr(s3, '_DELTASETS', {})

    def refused(match, era5=inside, d=gcm, **kw):
        with pytest.raises(ValueError, match=match):
            s3.load_delta_set(ctx, d, np.float64, era5=(era5, None), **kw)
        assert ctx.calls == [] and ctx.uploads == [] and s3._DELTASETS == {}

    refused('--bands', band=(0, 2))
    clean_mode.setattr(S, 'i_use_xesmf_regridding', 1)
    refused('i_use_xesmf_regridding')
    clean_mode.setattr(S, 'i_use_xesmf_regridding', 0)
    refused('1-D axes of their own', era5=_era5([-40.0, 0.0, 40.0], [10.0, 20.0, 30.0], two_d=True))
    # a regional source (not periodic, no pole rows) under targets that reach beyond it: the reference's two messages, raised
    # by regrid_tables when the plan of the first level variable is made
    regional = str(tmp_path / 'regional')
    synthetic.write_gcm_files(regional, nlat=24, nlon=48, plev=[100000.0, 50000.0, 10000.0], ocean=(6, 8))
    K.rewrite(regional, crop=(15.0, 65.0, 0.0, 60.0))
    refused('ERA5 dataset extends further North or South than GCM dataset!', era5=_era5([30.0, 70.0], [10.0, 20.0]), d=regional)
    refused('ERA5 dataset extends further East or West than GCM dataset!', era5=_era5([30.0, 40.0], [10.0, 80.0]), d=regional)
    for bad in ('ERA5', 'gcm', '', None, 1):
        clean_mode.setattr(S, 'delta_grid', bad)
        refused("must be 'era5' or 'source'")
    clean_mode.setattr(S, 'delta_grid', 'era5')
    clean_mode.setenv('PGW_DELTA_GRID', 'both')
    refused("must be 'era5' or 'source'")
    # the stages and the banded driver make the same check before they read a file
    with pytest.raises(ValueError, match="must be 'era5' or 'source'"):
        s3._stage_load(str(tmp_path / 'absent.nc'), str(tmp_path / 'out.nc'), gcm, None, True)
    clean_mode.setenv('PGW_DELTA_GRID', 'source')
    with pytest.raises(ValueError, match='--bands'):
        s3.pgw_for_era5_banded(str(tmp_path / 'absent.nc'), str(tmp_path / 'out.nc'), gcm, None, True, 0, 2, None, None)
    assert not (tmp_path / 'out.nc').exists()
