"""settings.delta_grid = 'source_points' and step_03's --rotate_winds without a GPU: the values on the argument surface, the
four points-plan entries in header, binding and library, every refusal before any library call (on the recording stand-in
of tests/function_recorder.py), the hand-over of both flags to the ranks of -p N, the paired window's bookkeeping on a fake
provider, and the conditions the cases of tests/source_points_cases.py exist for."""
import os
import re

import numpy as np
import pytest

import source_points_cases as Q
from function_recorder import RecordingContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('pgw_points_plan_create', 'pgw_points_plan_apply', 'pgw_points_plan_apply_wind', 'pgw_points_plan_destroy')
ENV = ('PGW_DELTA_GRID', 'PGW_ROTATE_WINDS')


@pytest.fixture
def clean_mode(monkeypatch):
    """PGW_DELTA_GRID and PGW_ROTATE_WINDS as the test found them afterwards (the command line sets them for its ranks)."""
    for name in ENV:
        monkeypatch.setenv(name, 'era5')                            # registered, so that whatever a test leaves is undone
        monkeypatch.delenv(name)
    return monkeypatch


def test_case_conditions():
    counts = Q.conditions()
    assert all(v > 0 for v in counts.values()), counts


def test_the_four_entries_are_declared_bound_and_exported():
    from pgw4era5_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and re.search(r'\bint %s\(' % name, hdr), name
    i, ll, vp, ip, dp = _lib._i, _lib._ll, _lib._vp, _lib._ip, _lib._dp
    tables = [ip, ip, dp, dp, ip, ip, dp, dp, ip]                   # pgw_regrid_points' nine, in its order
    assert _lib.SIGNATURES['pgw_regrid_points'][1][7:16] == tables
    assert _lib.SIGNATURES['pgw_points_plan_create'] == (i, [vp, i, i, ll] + tables + [i, i, ll, vp, vp, _lib._vpp])
    assert _lib.SIGNATURES['pgw_points_plan_apply'] == (i, [vp, vp, i, i, ll, vp, vp])
    assert _lib.SIGNATURES['pgw_points_plan_apply_wind'] == (i, [vp, vp, i, i, ll, vp, vp, vp, vp])
    assert _lib.SIGNATURES['pgw_points_plan_destroy'] == (i, [vp, vp])
    assert os.path.exists(_lib.LIB_PATH), 'libpgw_hip.so is not built'
    blob = open(_lib.LIB_PATH, 'rb').read()
    for name in ENTRIES:
        assert name.encode() + b'\0' in blob, '%s is not in the library' % name


def test_mode_parsing_and_the_environment_over_the_setting(clean_mode, capsys):
    from pgw4era5_amd import check_deltas, settings as S, step_03_apply_to_era as s3
    assert S.delta_grid == 'era5' and S.rotate_winds is None
    assert s3.delta_grid_mode() == 'era5' and s3.rotate_winds_request() is None
    clean_mode.setattr(S, 'delta_grid', 'source_points')
    assert s3.delta_grid_mode() == 'source_points'
    clean_mode.setenv('PGW_DELTA_GRID', 'source')
    assert s3.delta_grid_mode() == 'source'                         # the environment overrides the setting
    clean_mode.setenv('PGW_DELTA_GRID', 'source_points')
    clean_mode.setattr(S, 'delta_grid', 'era5')
    assert s3.delta_grid_mode() == 'source_points'
    clean_mode.setattr(S, 'rotate_winds', '39.25,-162')
    assert s3.rotate_winds_request() == '39.25,-162' and s3.delta_grid_mode() == 'source_points'
    clean_mode.setenv('PGW_ROTATE_WINDS', 'auto')
    assert s3.rotate_winds_request() == 'auto'
    for bad in ('points', 'source_point', 'SOURCE_POINTS'):
        clean_mode.setenv('PGW_DELTA_GRID', bad)
        with pytest.raises(ValueError, match="must be 'era5' or 'source'"):
            s3.delta_grid_mode()
    with pytest.raises(SystemExit):
        s3._cli(['--help'])
    out = capsys.readouterr().out
    assert 'source_points' in out and '--rotate_winds' in out
    with pytest.raises(SystemExit):
        s3._cli(['-i', 'a', '-o', 'b', '-d', 'c', '--delta_grid', 'points'])
    args = check_deltas.parse_args(['-i', 'a', '-g', 'b', '-d', 'c', '-o', 'd', '--delta_grid', 'source_points', '--rotate_winds'])
    assert args.delta_grid == 'source_points' and args.rotate_winds == 'auto'


def test_both_flags_reach_the_ranks_through_the_environment(clean_mode, tmp_path):
    """What `-p 2` starts are new processes: they inherit PGW_DELTA_GRID and PGW_ROTATE_WINDS while the command runs; the
    caller finds afterwards what it had."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    out = tmp_path / 'out'
    seen = []
    clean_mode.setattr(s3, '_run_cli', lambda args: seen.append(tuple(os.environ.get(k) for k in ENV)))
    base = ['-i', 'a', '-o', str(out), '-d', 'c', '-p', '2']
    s3._cli(base + ['--delta_grid', 'source_points', '--rotate_winds'])
    s3._cli(base + ['--delta_grid', 'source_points', '--rotate_winds', '43,-170'])
    s3._cli(base + ['--delta_grid', 'source_points'])
    assert all(k not in os.environ for k in ENV)
    clean_mode.setenv('PGW_ROTATE_WINDS', '6.55,0')
    s3._cli(base + ['--delta_grid', 'source_points'])
    s3._cli(base + ['--rotate_winds', 'auto'])
    assert seen == [('source_points', 'auto'), ('source_points', '43,-170'), ('source_points', None), ('source_points', '6.55,0'),
                    (None, 'auto')]
    assert os.environ['PGW_ROTATE_WINDS'] == '6.55,0' and 'PGW_DELTA_GRID' not in os.environ and not out.exists()


# ------------------------------------------------------------------ refusals
def _era5(layout='rotated', mapping=True):
    """An ERA5-like Dataset of 3 x 4 columns over Europe: 2-D lat / lon over (rlat, rlon) with a rotated mapping, the same
    columns as a cell list, or the mesh of two axes."""
    from pgw4era5_amd import ncio
    lat, lon = np.array([40.0, 45.0, 50.0]), np.array([5.0, 10.0, 15.0, 20.0])
    la, lo = np.meshgrid(lat, lon, indexing='ij')
    ds = ncio.Dataset()
    if layout == 'rotated':
        ds['lat'], ds['lon'] = ncio.Field(la, ('rlat', 'rlon')), ncio.Field(lo, ('rlat', 'rlon'))
        dims = ('time', 'rlat', 'rlon')
        if mapping:
            ds['rotated_pole'] = ncio.Field(np.array(b'', dtype='S1'), (), attrs=dict(
                grid_mapping_name='rotated_latitude_longitude', grid_north_pole_latitude=39.25, grid_north_pole_longitude=-162.0))
    elif layout == 'cells':
        ds['lat'], ds['lon'] = ncio.Field(la.ravel(), ('cell',)), ncio.Field(lo.ravel(), ('cell',))
        dims = ('time', 'cell')
    else:
        ds['lat'], ds['lon'] = ncio.Field(lat, ('lat',)), ncio.Field(lon, ('lon',))
        dims = ('time', 'lat', 'lon')
    ds['FR_LAND'] = ncio.Field(np.zeros((1,) + la.shape if len(dims) == 3 else (1, la.size)), dims)
    return ds


def _edit(path, var, **changes):
    from pgw4era5_amd import ncio
    ds = ncio.open_dataset(path)
    f = ds[var]
    attrs = dict(f.attrs, **changes.get('attrs', {}))
    if 'time' in changes:
        ds['time'] = ncio.Field(changes['time'], ('time',), attrs=ds['time'].attrs)
    coords = {d: np.asarray(ds[d].values) for d in f.dims if d in ds}
    ds[var] = ncio.Field(np.asarray(f.values), f.dims, coords, attrs)
    ncio.to_netcdf(ds, path)


def test_every_refusal_comes_before_any_library_call(clean_mode, tmp_path):
    """--rotate_winds with 'era5' (rotate in step_02) and with 'source', on a mesh file (nothing to rotate), --bands, the xESMF
    setting, a marker already on the source (double rotation), ua / va on different time axes, step_02's pole-parsing errors,
    a source that does not cover the targets: ValueError with no pgw_* call recorded and nothing uploaded."""
    import shutil
    from pgw4era5_amd import settings as S, step_03_apply_to_era as s3, synthetic
    ctx = RecordingContext()
    ctx.device = 0
    gcm = str(tmp_path / 'gcm')
    synthetic.write_gcm_files(gcm, nlat=5, nlon=8, plev=[100000.0, 50000.0, 10000.0], ocean=(6, 8))
    clean_mode.setattr(s3, '_DELTASETS', {})

    def refused(match, era5=None, d=gcm, mode='source_points', rotate=None, **kw):
        clean_mode.setattr(S, 'delta_grid', mode)
        clean_mode.setattr(S, 'rotate_winds', rotate)
        with pytest.raises(ValueError, match=match):
            s3.load_delta_set(ctx, d, np.float64, era5=(_era5() if era5 is None else era5, None), **kw)
        assert ctx.calls == [] and ctx.uploads == [] and s3._DELTASETS == {}

    refused('rotate in step_02', mode='era5', rotate='auto')
    refused("--rotate_winds with delta_grid = 'source'", mode='source', rotate='auto', era5=_era5('mesh'))
    refused('nothing to rotate', rotate='auto', era5=_era5('mesh'))
    refused('nothing to rotate', rotate='39.25,-162', era5=_era5('mesh'))
    refused('--bands', band=(0, 2))
    clean_mode.setattr(S, 'i_use_xesmf_regridding', 1)
    refused('i_use_xesmf_regridding')
    clean_mode.setattr(S, 'i_use_xesmf_regridding', 0)
    # step_02's pole-parsing errors
    refused("takes 'auto' or POLE_LAT,POLE_LON", rotate='north')
    refused("takes 'auto' or POLE_LAT,POLE_LON", rotate='39.25')
    refused('is not a position in degrees', rotate='139.25,-162')
    refused('no rotated mapping found', rotate='auto', era5=_era5(mapping=False))
    refused('no rotated mapping found', rotate='auto', era5=_era5('cells'))
    # the ua / va pair
    marked = str(tmp_path / 'marked')
    shutil.copytree(gcm, marked)
    _edit(os.path.join(marked, 'va_delta.nc'), 'va', attrs=dict(wind_components='grid_relative'))
    refused('double rotation', rotate='auto', d=marked)
    shifted = str(tmp_path / 'shifted')
    shutil.copytree(gcm, shifted)
    t = np.asarray(__import__('pgw4era5_amd.ncio', fromlist=['x']).open_dataset(os.path.join(shifted, 'va_delta.nc'))['time'].values)
    _edit(os.path.join(shifted, 'va_delta.nc'), 'va', time=t + np.timedelta64(1, 'D'))
    refused('different time axes', rotate='auto', d=shifted)
    # a regional source under targets that reach beyond it: the reference's messages, from regrid_tables
    regional = str(tmp_path / 'regional')
    synthetic.write_gcm_files(regional, nlat=24, nlon=48, plev=[100000.0, 50000.0, 10000.0], ocean=(6, 8))
    import source_delta_cases as K
    K.rewrite(regional, crop=(15.0, 45.0, 0.0, 60.0))
    refused('ERA5 dataset extends further North or South than GCM dataset!', d=regional)
    K.rewrite(regional, crop=(15.0, 45.0, 0.0, 12.0))
    with pytest.raises(ValueError, match='ERA5 dataset extends further'):
        s3.load_delta_set(ctx, regional, np.float64, era5=(_era5('cells'), None))
    assert ctx.calls == [] and ctx.uploads == []
    # the stages make the mode check before they read a file, the command line before it makes a directory
    clean_mode.setattr(S, 'rotate_winds', 'auto')
    clean_mode.setattr(S, 'delta_grid', 'era5')
    with pytest.raises(ValueError, match='rotate in step_02'):
        s3._stage_load(str(tmp_path / 'absent.nc'), str(tmp_path / 'out.nc'), gcm, None, True)
    clean_mode.setattr(S, 'rotate_winds', None)
    out = tmp_path / 'out'
    args = ['-i', str(tmp_path), '-o', str(out), '-d', gcm]
    for extra, match in ((['--rotate_winds'], 'rotate in step_02'), (['--rotate_winds', '--delta_grid', 'source'], "delta_grid = 'source'"),
                         (['--delta_grid', 'source_points', '--bands'], '--bands'),
                         (['--delta_grid', 'source_points', '--rotate_winds', 'x,y'], "takes 'auto' or POLE_LAT,POLE_LON")):
        with pytest.raises(ValueError, match=match):
            s3._cli(args + extra)
    assert not out.exists() and all(k not in os.environ for k in ENV)
    assert ctx.calls == [] and ctx.uploads == []


# ------------------------------------------------------------------ the paired window
class FakePair:
    """A paired provider that writes (record, component) into the arrays it is handed and counts its launches."""
    variables = ('ua', 'va')
    nrec, rec_shape = 12, (2, 3, 4)

    def __init__(self):
        self.launches, self.freed = [], 0

    def device_pair(self, r, out_u, out_v):
        self.launches.append(r)
        for k, out in enumerate((out_u, out_v)):
            out.ctx.mem[out.ptr][...] = 10.0 * r + k

    def free(self):
        self.freed += 1


def test_the_paired_window_moves_in_lockstep(clean_mode):
    """DeltaSet over a paired provider: a miss of either variable fills record r of both with ONE launch, the other
    variable's request is a hit; both windows hold the same records in the same order, never more than WINDOW; the least
    recently used slot of both is reused (the same DeviceArrays); an evicted record comes back with one more launch."""
    import source_delta_cases as K
    from pgw4era5_amd import step_03_apply_to_era as s3
    ctx = RecordingContext()
    pair = FakePair()
    times = K.monthly_axis()
    dset = s3.DeltaSet(ctx, {'ua': pair, 'va': pair}, times, np.array([85000.0, 50000.0]), np.float64, resident=False)
    assert set(dset._src) == {'ua', 'va'} and dset.dev == {}
    syncs = []
    ctx.sync = lambda: syncs.append(1)
    W4 = s3.DeltaSet.WINDOW
    owners = {}
    for n, r in enumerate([0, 1, 1, 2, 3, 0, 4, 5, 1, 5, 0, 2]):
        first, second = ('va', 'ua') if n % 2 else ('ua', 'va')      # either variable may be the one that misses
        before = len(pair.launches)
        missed = r not in dset._cache[first]
        a = dset.rec(first, r)
        assert len(pair.launches) == before + (1 if missed else 0)
        b = dset.rec(second, r)
        assert len(pair.launches) == before + (1 if missed else 0)  # the other variable's request is a hit
        ku, kv = list(dset._cache['ua']), list(dset._cache['va'])
        assert ku == kv and len(ku) <= W4 and ku[-1] == r            # lockstep: same records, same order, r most recent
        vals = {first: a, second: b}
        assert float(ctx.mem[vals['ua'].ptr].ravel()[0]) == 10.0 * r and float(ctx.mem[vals['va'].ptr].ravel()[0]) == 10.0 * r + 1
        assert vals['ua'].ptr != vals['va'].ptr
        owners.setdefault('ua', set()).add(vals['ua'].ptr)
        owners.setdefault('va', set()).add(vals['va'].ptr)
    assert pair.launches == [0, 1, 2, 3, 4, 5, 1, 2]                 # 1 and 2 were evicted and came back
    assert len(owners['ua']) == W4 and len(owners['va']) == W4       # the slots are reused, none is added
    assert syncs == []
    dset.free()
    assert pair.freed == 2 and dset._cache == {}                     # met under both names: free() may be repeated
