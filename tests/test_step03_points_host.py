"""step_03 on files with 2-D coordinates or a cell list, without a GPU: the layout helper, the errors that must come before
any library call (on the recording stand-in of tests/function_recorder.py), the default layout of
synthetic.write_case_files, and the conditions the cases of tests/points_file_cases.py exist for."""
import datetime as dt
import hashlib
import os

import numpy as np
import pytest

import points_file_cases as P
from function_recorder import RecordingContext


@pytest.fixture
def clean_mode(monkeypatch):
    monkeypatch.setenv('PGW_DELTA_GRID', 'era5')                    # registered, so that whatever a test leaves is undone
    monkeypatch.delenv('PGW_DELTA_GRID')
    return monkeypatch


def test_case_conditions():
    assert P.conditions()


def _ds(lat_dims, lon_dims, shapes):
    from pgw4era5_amd import ncio
    ds = ncio.Dataset()
    ds['lat'] = ncio.Field(np.zeros([shapes[d] for d in lat_dims]), lat_dims)
    ds['lon'] = ncio.Field(np.zeros([shapes[d] for d in lon_dims]), lon_dims)
    return ds


def test_layout_helper():
    from pgw4era5_amd import step_03_apply_to_era as s3
    n = dict(lat=3, lon=4, rlat=3, rlon=4, cell=5, time=1, y=3, x=4)
    assert s3.era_layout(_ds(('lat',), ('lon',), n)) == ('lat', 'lon')
    assert s3.era_layout(_ds(('rlat', 'rlon'), ('rlat', 'rlon'), n)) == ('rlat', 'rlon')
    assert s3.era_layout(_ds(('cell',), ('cell',), n)) == ('cell',)
    assert s3.is_mesh(('lat', 'lon')) and not s3.is_mesh(('rlat', 'rlon')) and not s3.is_mesh(('cell',))
    for bad in (_ds(('rlat', 'rlon'), ('rlon', 'rlat'), n), _ds(('lat',), ('rlat', 'rlon'), n), _ds(('y', 'x'), ('lon',), n)):
        with pytest.raises(ValueError, match='neither two 1-D axes of a mesh nor point-wise coordinates'):
            s3.era_layout(bad)
    with pytest.raises(ValueError, match='one dimension .a cell list. or two'):
        s3.era_layout(_ds(('time', 'rlat', 'rlon'), ('time', 'rlat', 'rlon'), n))
    d = s3.layout_dims(('rlat', 'rlon'))
    assert d == dict(d3=('time', 'rlat', 'rlon'), d4=('time', 'level', 'rlat', 'rlon'), so=('time', 'soil1', 'rlat', 'rlon'))
    assert s3.layout_dims(('lat', 'lon'))['d4'] == ('time', 'level', 'lat', 'lon')
    # a cell list is a grid of one row: views of the same memory, there and back
    v = np.arange(30.0).reshape(1, 6, 5)
    g = s3._as_grid(v, ('cell',))
    assert g.shape == (1, 6, 1, 5) and np.shares_memory(g, v) and s3._as_file(g, ('cell',)).shape == v.shape
    assert s3._as_grid(v, ('rlat', 'rlon')) is v and s3._as_file(v, ('lat', 'lon')) is v


def _point_file(tmp_path, name='rotated 7x9', **edit):
    from pgw4era5_amd import synthetic
    case, layout = P.file_case(name, P.INSTANTS[0], np.float64)
    return synthetic.write_case_files(case, str(tmp_path / 'era'), str(tmp_path / 'deltas'), layout=layout), str(tmp_path / 'deltas')


def test_file_layout_reads_the_header(tmp_path):
    from pgw4era5_amd import ncio, step_03_apply_to_era as s3
    path, _ = _point_file(tmp_path)
    assert s3.file_layout(path) == ('rlat', 'rlon') == s3.era_layout(ncio.open_dataset(path, decode_times=False))
    path, _ = _point_file(tmp_path / 'c', 'cells 65')
    assert s3.file_layout(path) == ('cell',)
    ds = ncio.open_dataset(path, decode_times=False)
    assert ds['T'].dims == ('time', 'level', 'cell') and ds['lat'].dims == ('cell',) and ds['T'].shape == (1, P.NLEV, 65)
    dd = ncio.open_dataset(os.path.join(str(tmp_path / 'c' / 'deltas'), 'ta_delta.nc'))
    assert dd['ta'].dims == ('time', 'plev', 'cell') and dd['lat'].dims == ('cell',)


def test_errors_come_before_any_library_call(clean_mode, tmp_path):
    """--bands on a point-wise file, lat over (rlat, rlon) beside lon over (rlon, rlat), a field that lacks a horizontal
    dimension: ValueError with no pgw_* call recorded and nothing uploaded."""
    from pgw4era5_amd import ncio, settings as S, step_03_apply_to_era as s3
    ctx = RecordingContext()
    ctx.device = 0
    clean_mode.setattr(s3, 'default_context', lambda: ctx)
    clean_mode.setattr(s3, '_DELTASETS', {})
    clean_mode.setattr(S, 'i_debug', -1)
    clean_mode.setenv('PGW_IO_RAW', '0')
    path, deltas = _point_file(tmp_path)
    out = str(tmp_path / 'out.nc')

    def untouched():
        assert ctx.calls == [] and ctx.uploads == [] and s3._DELTASETS == {} and not os.path.exists(out)

    with pytest.raises(ValueError, match='--bands on a point-wise file is not built'):
        s3.pgw_for_era5_banded(path, out, deltas, P.INSTANTS[0], True, 0, 2, None, None)
    untouched()
    with pytest.raises(ValueError, match='--bands on a point-wise file is not built'):
        s3._cli(['-i', os.path.dirname(path), '-o', str(tmp_path / 'o'), '-d', deltas, '-f', '2006072006', '-l', '2006072006',
                 '-t', '--bands'])
    untouched()
    assert not (tmp_path / 'o').exists()
    # lat over (rlat, rlon) beside lon over (rlon, rlat)
    ds = ncio.open_dataset(path, decode_times=False)
    ds['lon'] = ncio.Field(np.ascontiguousarray(ds['lon'].values.T), ('rlon', 'rlat'), {}, ds['lon'].attrs)
    crossed = str(tmp_path / 'crossed.nc')
    ncio.to_netcdf(ds, crossed)
    with pytest.raises(ValueError, match='neither two 1-D axes of a mesh nor point-wise coordinates'):
        s3._stage_load(crossed, out, deltas, P.INSTANTS[0], True)
    untouched()
    # a field that lacks one of the horizontal dimensions
    ds = ncio.open_dataset(path, decode_times=False)
    ds['PS'] = ncio.Field(ds['PS'].values[:, :, 0], ('time', 'rlat'), {}, ds['PS'].attrs)
    short = str(tmp_path / 'short.nc')
    ncio.to_netcdf(ds, short)
    with pytest.raises(ValueError, match="PS lies over .'time', 'rlat'.; the horizontal layout of the file asks for"):
        s3._stage_load(short, out, deltas, P.INSTANTS[0], True)
    untouched()


def _plain_case(dtype):
    """A case whose arrays are halves of whole numbers: the bytes of its files depend on the writer alone."""
    nlev, nlat, nlon, nsoil, nplev = 3, 2, 4, 2, 2

    def a(*shape, off=0.0):
        return (np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) * 0.5 + off).astype(dtype)
    era = dict(ak=np.arange(nlev + 1) * 10.0, bk=np.arange(nlev + 1) / nlev, soil1=np.array([0.25, 1.5]),
               PS=a(1, nlat, nlon, off=1000.0), FIS=a(1, nlat, nlon), T=a(1, nlev, nlat, nlon, off=200.0),
               QV=a(1, nlev, nlat, nlon), U=a(1, nlev, nlat, nlon, off=-5.0), V=a(1, nlev, nlat, nlon, off=3.0),
               T_SKIN=a(1, nlat, nlon, off=280.0), T_SO=a(1, nsoil, nlat, nlon, off=270.0), FR_LAND=a(1, nlat, nlon) * 0 + 1,
               FR_SEA_ICE=a(1, nlat, nlon) * 0)
    deltas = {k: a(12, nplev, nlat, nlon, off=i) for i, k in enumerate(('ta', 'hur', 'ua', 'va', 'zg'))}
    deltas.update({k: a(12, nlat, nlon, off=i) for i, k in enumerate(('tas', 'hurs', 'ts', 'tos', 'siconc', 'ps_hist'))})
    times = np.array(['1995-%02d-15T12:00:00' % (m + 1) for m in range(12)], dtype='datetime64[s]')
    return dict(era=era, deltas=deltas, delta_times=times, plev=np.array([85000.0, 30000.0]), target_dt=dt.datetime(2006, 8, 2, 3),
                lat=np.array([-10.0, 10.0]), lon=np.array([0.0, 90.0, 180.0, 270.0]))


# sha256 over the names and bytes of the ERA5 file and the eleven delta files write_case_files wrote for _plain_case before it
# knew layouts
BEFORE = {'float64': 'b11e86c7c46a853d8a872479a8185e7f68bf129792f74633e68ddd8a02849279',
          'float32': '2d372b8761aeeb1d311468baeefadec92ae6b9412785533188d3f79ab46f19a6'}


def _digest(*dirs):
    h = hashlib.sha256()
    for root in dirs:
        for n in sorted(os.listdir(root)):
            h.update(n.encode())
            h.update(open(os.path.join(root, n), 'rb').read())
    return h.hexdigest()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_the_default_layout_writes_the_bytes_it_wrote(tmp_path, dtype):
    from pgw4era5_amd import synthetic
    for leg, kw in (('default', {}), ('named', dict(layout='mesh'))):
        era, deltas = str(tmp_path / leg / 'era'), str(tmp_path / leg / 'deltas')
        synthetic.write_case_files(_plain_case(np.dtype(dtype)), era, deltas, **kw)
        assert len(os.listdir(deltas)) == 11
        assert _digest(era, deltas) == BEFORE[dtype], leg
    with pytest.raises(ValueError, match="layout must be 'mesh', 'rotated' or 'cells'"):
        synthetic.write_case_files(_plain_case(np.dtype(dtype)), str(tmp_path / 'x'), str(tmp_path / 'y'), layout='curvilinear')
