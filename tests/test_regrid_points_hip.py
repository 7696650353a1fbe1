"""GPU checks of the default branch's regridding onto point-wise targets (`pgw_regrid_points`: k_zonal_mean_rows,
k_regrid_points; `functions.regrid_points`; `functions.regrid_lat_lon` and the step_02 command line with a 2-D target).

The definition of correct is `statement` of tests/test_regrid_points_host.py, tied there to scipy's interp1d composition and
to k_regrid's separable computation.  PARITY WITH XARRAY ITSELF IS UNPINNED.  Wherever no latitude bracket names a pole row
the kernel is held to the statement's BITS.  Where one does, the kernel's lane-strided zonal mean and numpy's differ by at
most nlon_s * eps * max|row|, and both passes have weights in [0, 1]: |difference| <= (nlon_s + 8) * eps * max|v|, eps that
of the storage type.  Cases that claim bit equality have at most 0.10 of their targets under the bound instead."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import extpar_cases as XC                                                             # noqa: E402
import test_extpar_adapt_hip as XA                                                    # noqa: E402
import test_regrid_points_host as H                                                   # noqa: E402
from pgw4era5_amd import _lib, ncio, settings, synthetic
from pgw4era5_amd import functions as F
from pgw4era5_amd.device import default_context
from pgw4era5_amd.postproc_cosmo import extpar_adapt as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
NTARG = [1, 63, 64, 65, 257, 511, 512, 513, 1030]
_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


def points(c, dtype):
    """functions.regrid_points on the case's field stored as `dtype` -> (nfield, ntarg)."""
    got = F.regrid_points(c.field.astype(dtype), c.slat, c.slon, c.tlat, c.tlon)
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == (c.nfield,) + c.tlat.shape
    return got.reshape(c.nfield, -1)


def check(got, c, dtype, max_pole_share=0.10):
    """Bits where no bracket names a pole row, the derived bound where one does, NaN masks equal."""
    want = c.want(dtype)
    assert c.pole.mean() <= max_pole_share
    H.same_bits(got[:, ~c.pole], want[:, ~c.pole])
    if c.pole.any():
        g, w = got[:, c.pole].astype(np.float64), want[:, c.pole].astype(np.float64)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
        bound = (c.nlon_s + 8) * float(np.finfo(dtype).eps) * np.nanmax(np.abs(c.field))
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= bound).all(), (np.abs(g[ok] - w[ok]).max(), bound)


# ----------------------------------------------------------------------------------------------- 1. the statement
@pytest.mark.parametrize('ntarg', NTARG)
@pytest.mark.parametrize('kind', ['asc0', 'desc180', 'regional'])
def test_rotated_targets_equal_the_statement(kind, ntarg):
    """The leading points of a rotated 24 x 48 grid on a 48 x 96 source: no pole row, every bit is pinned."""
    for nfield in (1, 3, 40):
        c = H.rotated_case(kind, 48, 96, ntarg, nfield)
        for dtype in DTYPES:
            check(points(c, dtype), c, dtype, max_pole_share=0.0)


@pytest.mark.parametrize('ntarg', NTARG)
@pytest.mark.parametrize('source', ['asc0 5x8', 'desc180 5x8', 'asc0 48x96', 'desc180 48x96', 'regional 48x96'])
def test_random_point_lists_equal_the_statement(source, ntarg):
    kind, shape = source.split()
    nlat_s, nlon_s = (int(n) for n in shape.split('x'))
    for nfield in (1, 3, 40):
        c = H.random_case(kind, nlat_s, nlon_s, ntarg, nfield)
        for dtype in DTYPES:
            check(points(c, dtype), c, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_ragged_and_empty_plane_slices(dtype):
    """131071 targets (512 blocks, the last one ragged) and 40 planes: 16 z-slices of 3 planes - 13 full, one with a single
    plane, two empty.  With few targets every plane is its own slice (the launch wants 8192 blocks), so the walk over
    several planes of a slice, its ragged end and the empty slice take this many targets."""
    gz, per, sizes = H.slices(40, 131071)
    assert (gz, per) == (16, 3) and sizes == [3] * 13 + [1, 0, 0]
    slat, slon = H.source('regional', 48, 96)
    rng = np.random.default_rng(40)
    c = H.Case(H._field(rng, (40, 48, 96)), slat, slon, rng.uniform(slat.min(), slat.max(), 131071),
               rng.uniform(slon.min(), slon.max(), 131071))
    assert not c.pole.any()
    check(points(c, dtype), c, dtype, max_pole_share=0.0)


# ----------------------------------------------------------------------------------------------- 2. regrid_field
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('which', ['37x72', '7x9'])
def test_mesh_as_points_equals_regrid_field(which, dtype):
    """Pole rows included: both entries take the pole values from k_zonal_mean_rows."""
    c = H.mesh_case(which)
    tlat, tlon = c.mesh
    f = c.field.astype(dtype)
    want = F.regrid_field(f, c.slat, c.slon, tlat, tlon)
    la2, lo2 = np.meshgrid(tlat, tlon, indexing='ij')
    got = F.regrid_points(f, c.slat, c.slon, la2, lo2)
    assert got.shape == want.shape == (3, len(tlat), len(tlon))
    H.same_bits(got, want)


# ----------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', H.LAYOUT_CASES)
def test_layouts(name, dtype):
    """A block across the periodic seam, a block holding both poles, a block of pole brackets only, targets in random order,
    neighbouring targets over five blocks with a ragged last one."""
    c = H.layout_case(name)
    check(points(c, dtype), c, dtype, max_pole_share=1.0)


# ----------------------------------------------------------------------------------------------- 4. ground truth
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['asc0', 'desc180', 'regional'])
def test_linear_field_is_reproduced(kind, dtype):
    """f = a + b lat + c lon on targets inside [src_lon[0], src_lon[-1]] and between the edge rows: three lerps of at most
    three roundings each (the statement reaches 1.9 eps max|f| on the CPU) - within 16 eps max|f|, eps of the storage type
    (a float32 field is the linear one rounded once per value; the weights are convex)."""
    slat, slon = H.source(kind, 48, 96)
    rng = np.random.default_rng(11)
    tlat, tlon = rng.uniform(slat.min(), slat.max(), 1030), rng.uniform(slon.min(), slon.max(), 1030)

    def f(lat, lon):
        return 250.0 + 0.37 * lat - 0.11 * lon
    field = f(slat[:, None], slon[None, :])[None].astype(dtype)
    got = F.regrid_points(field, slat, slon, tlat, tlon)
    assert got.shape == (1, 1030) and got.dtype == dtype
    bound = 16 * float(np.finfo(dtype).eps) * np.abs(field).max()
    assert np.abs(got[0].astype(np.float64) - f(tlat, tlon)).max() <= bound


# ----------------------------------------------------------------------------------------------- 5. NaN
@pytest.mark.parametrize('dtype', DTYPES)
def test_nan_corners_pole_rows_and_target_coordinates(dtype):
    c0 = H.random_case('asc0', 48, 96, 1030, 3)
    t0 = c0.tb
    g1 = int(np.flatnonzero(~c0.pole)[100])                         # a corner of an inner target
    g2 = int(np.flatnonzero(t0['lat_hi'] == 48)[0])                  # an entry of the north row, under a target at the pole
    n1, n2 = (int(t0['lat_lo'][g1]), int(t0['lon_hi'][g1])), (47, int(t0['lon_lo'][g2]))
    f = c0.field.copy()
    f[1][n1] = np.nan
    f[2][n2] = np.nan                                                # skipped by the pole mean
    c = H.Case(f, c0.slat, c0.slon, c0.tlat, c0.tlon)
    tb = c.tb
    corners = [(tb['lat_lo'], tb['lon_lo']), (tb['lat_lo'], tb['lon_hi']), (tb['lat_hi'], tb['lon_lo']), (tb['lat_hi'], tb['lon_hi'])]
    got = points(c, dtype)
    check(got, c, dtype)
    for plane, (r, col) in ((1, n1), (2, n2)):
        touch = np.zeros(c.ntarg, dtype=bool)
        for rows, cols in corners:
            touch |= (rows == r) & (cols == col)
        assert touch.any() and np.array_equal(np.isnan(got[plane]), touch)           # exactly the targets that touch it
    assert not np.isnan(got[0]).any()
    north = (tb['lat_hi'] == 48) & (tb['lon_lo'] != n2[1]) & (tb['lon_hi'] != n2[1])
    assert north.any() and not np.isnan(got[2][north]).any()
    # a NaN target coordinate gives NaN by the arithmetic; the extremes that decide pole rows and copies are numpy's, which a
    # NaN turns off - on a regional source nothing else depends on them
    r = H.rotated_case('regional', 48, 96, 513)
    for name in ('tlat', 'tlon'):
        t = dict(tlat=r.tlat.copy(), tlon=r.tlon.copy())
        t[name][[0, 77, 512]] = np.nan
        cn = H.Case(r.field, r.slat, r.slon, t['tlat'], t['tlon'])
        got = points(cn, dtype)
        H.same_bits(got, cn.want(dtype))
        assert np.isnan(got[:, [0, 77, 512]]).all() and np.isnan(got).sum() == 3 * 3


# ----------------------------------------------------------------------------------------------- 6. errors
def test_argument_errors_leave_the_output_alone():
    ctx = default_context()
    c = H.random_case('asc0', 5, 8, 65, 3)
    assert c.pole.any() and c.tb['south_row'] == 0 and c.tb['north_row'] == 4
    src = ctx.to_device(c.field)
    sentinel = np.full((3, 65), 7.25)
    out = ctx.to_device(sentinel)
    base = {k: np.ascontiguousarray(v) for k, v in c.tb.items() if isinstance(v, np.ndarray)}
    base['oob'] = np.ascontiguousarray(base['lat_oob'] | base['lon_oob'], dtype=np.int32)

    def rc(dtype=_lib.PGW_F64, nfield=3, nlat_s=5, nlon_s=8, ntarg=65, s=src.ptr, o=out.ptr, south=0, north=4, null=None, **edit):
        t = {k: v.copy() for k, v in base.items()}
        for k, (i, v) in edit.items():
            t[k][i] = v
        p = {k: (None if k == null else v.ctypes.data_as(_ip if v.dtype == np.int32 else _dp)) for k, v in t.items()}
        return ctx.lib.pgw_regrid_points(ctx.handle, dtype, nfield, nlat_s, nlon_s, ntarg, s, p['lat_lo'], p['lat_hi'], p['lat_dx'],
                                         p['lat_Dx'], p['lon_lo'], p['lon_hi'], p['lon_dx'], p['lon_Dx'], p['oob'], south, north, o)
    inner = int(np.flatnonzero(~c.pole)[0])
    sp, npole = int(np.flatnonzero(c.tb['lat_lo'] == -1)[0]), int(np.flatnonzero(c.tb['lat_hi'] == 5)[0])
    bad = [rc(dtype=7), rc(nfield=0), rc(nfield=-3), rc(ntarg=0), rc(ntarg=-65), rc(nlat_s=1), rc(nlon_s=1), rc(nlat_s=0), rc(s=None),
           rc(o=None), rc(null='lat_lo'), rc(null='lon_Dx'), rc(null='oob'),
           rc(lat_lo=(inner, -2)), rc(lat_hi=(inner, 6)), rc(lon_lo=(inner, -1)), rc(lon_hi=(inner, 8)), rc(lon_lo=(64, 8)),
           rc(south=-1), rc(north=-1), rc(south=5), rc(north=5)]
    assert bad == [_lib.PGW_ERR_ARG] * len(bad), bad
    ctx.sync()
    np.testing.assert_array_equal(out.numpy(), sentinel)                             # nothing ran
    with pytest.raises(ValueError, match='pgw_regrid_points'):
        ctx._check(rc(lat_lo=(inner, -2)))
    # an index out of range in an oob target is not read; a pole row may go unnamed when no valid target names it
    assert rc(oob=(inner, 1), lat_lo=(inner, -99), lon_hi=(inner, 12345)) == _lib.PGW_OK
    assert np.isnan(out.numpy()[:, inner]).all()
    assert rc(south=-1, oob=(np.flatnonzero(c.tb['lat_lo'] == -1), 1)) == _lib.PGW_OK
    assert rc() == _lib.PGW_OK and sp != npole
    got = out.numpy()
    check(got, c, np.float64, max_pole_share=1.0)


# ----------------------------------------------------------------------------------------------- 7. files
def _write_ts(gcm, nlat, nlon, dtype, seed=0):
    """ts_delta.nc / ts_historical.nc on a Gaussian-like global grid, 12 monthly records, smooth plus noise, never 0."""
    os.makedirs(gcm, exist_ok=True)
    slat, slon = H.source('asc0', nlat, nlon)
    rng = np.random.default_rng(seed)
    ts = (1.5 + np.cos(np.deg2rad(slat))[None, :, None] * (1 + 0.2 * np.sin(np.deg2rad(3 * slon)))[None, None, :]
          + 0.1 * rng.standard_normal((12, nlat, nlon))).astype(dtype)
    times = np.array(['1995-%02d-15T12:00:00' % (m + 1) for m in range(12)], dtype='datetime64[s]')
    for base in settings.file_name_bases.values():
        ds = ncio.Dataset(attrs=dict(title='ts on a regular grid'))
        ds['time'] = ncio.Field(times, ('time',))
        ds['lat'] = ncio.Field(slat, ('lat',), attrs=dict(units='degrees_north'))
        ds['lon'] = ncio.Field(slon, ('lon',), attrs=dict(units='degrees_east'))
        ds['ts'] = ncio.Field(ts, ('time', 'lat', 'lon'), attrs=dict(units='K'))
        ncio.to_netcdf(ds, os.path.join(gcm, base.format('ts')))


def _chain(tmp_path, gcm, shape, tb_dtype):
    """step_02 regridding -e EXTPAR -v ts under default settings, then extpar_adapt; everything against the statement."""
    from pgw4era5_amd import step_02_preproc_deltas as s2
    assert settings.i_use_xesmf_regridding == 0
    info = synthetic.make_extpar(str(tmp_path / 'extpar.nc'), shape[0], shape[1], dtype=tb_dtype, time_axis=True, fill='_FillValue')
    ext = ncio.open_dataset(info['path'], decode_times=False, decode_mask_scale=False)
    lat2, lon2 = np.asarray(ext['lat'].values), np.asarray(ext['lon'].values)
    deltas = tmp_path / 'extpar_deltas'
    s2.main(['regridding', '-i', str(gcm), '-o', str(deltas), '-e', info['path'], '-v', 'ts'])
    src = ncio.open_dataset(os.path.join(str(gcm), 'ts_delta.nc'))
    vals = np.asarray(src['ts'].values)
    tb = H.tables(src['lat'].values, src['lon'].values, lat2, lon2)
    assert tb['south_row'] == tb['north_row'] == -1                                  # no pole row: every bit is pinned
    want_ts = H.statement(vals, tb).reshape((12,) + shape)
    for base in settings.file_name_bases.values():
        got = ncio.open_dataset(str(deltas / base.format('ts')))
        assert got['ts'].dims == ('time', 'rlat', 'rlon') and got['ts'].dtype == vals.dtype
        assert got['lat'].dims == got['lon'].dims == ('rlat', 'rlon') and got['ts'].attrs.get('units') == src['ts'].attrs.get('units')
        np.testing.assert_array_equal(got['lat'].values, lat2)
        np.testing.assert_array_equal(got['lon'].values, lon2)
        ts = np.asarray(got['ts'].values)
        H.same_bits(ts, want_ts)
        assert not np.isnan(vals).any() and not (vals == 0.0).any()
        assert not (ts == 0.0).any() and not np.isnan(ts).any()                     # no holes
    before = open(info['path'], 'rb').read()
    A.extpar_adapt(info['path'], str(deltas))
    want = XC.statement(info['T_CL'], want_ts, info['mask_values'])[0]
    got = XA.t_cl_words(info['path']).astype(tb_dtype)
    assert got.shape == (1,) + shape and XC.same_bits(got, want, raw=info['masked'])
    changed = ~info['masked']
    assert (XC.uview(got)[changed] != XC.uview(info['T_CL'])[changed]).mean() > 0.99
    assert XA.outside_t_cl(info['path'], before) == before
    return info, deltas


@pytest.mark.parametrize('shape', [(7, 9), (33, 65)], ids=['7x9', '33x65'])
def test_chain_from_step02_under_default_settings(tmp_path, shape):
    gcm = tmp_path / 'gcm'
    synthetic.write_gcm_files(str(gcm), nlat=24, nlon=48, plev=[85000.0, 50000.0])
    _chain(tmp_path, gcm, shape, np.float32)
    # regrid_lat_lon itself: every horizontal variable through regrid_points, laid out on the target's dimensions
    ds = ncio.open_dataset(str(gcm / 'ta_delta.nc'))
    ext = ncio.open_dataset(str(tmp_path / 'extpar.nc'), decode_times=False)
    out = F.regrid_lat_lon(ds, ext, 'ta')
    assert out['ta'].dims == ('time', 'plev', 'rlat', 'rlon') and out['ta'].shape == (12, 2) + shape
    H.same_bits(np.asarray(out['ta'].values),
                F.regrid_points(np.asarray(ds['ta'].values), ds['lat'].values, ds['lon'].values, ext['lat'].values, ext['lon'].values))
    np.testing.assert_array_equal(out['plev'].values, ds['plev'].values)


def test_chain_on_a_fine_source(tmp_path):
    """192 x 384 (0.94 deg): the resolution at which the xESMF branch leaves holes; this branch cannot."""
    gcm = tmp_path / 'gcm'
    _write_ts(str(gcm), 192, 384, np.float32)
    _chain(tmp_path, gcm, (33, 65), np.float64)


def test_step02_command_line(tmp_path):
    gcm = tmp_path / 'gcm'
    _write_ts(str(gcm), 24, 48, np.float64)
    info, deltas = _chain(tmp_path, gcm, (7, 9), np.float32)
    outd = tmp_path / 'by_command'
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'pgw4era5_amd.step_02_preproc_deltas', 'regridding', '-i', str(gcm), '-o', str(outd),
                        '-e', info['path'], '-v', 'ts'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for base in settings.file_name_bases.values():
        a, b = ncio.open_dataset(str(deltas / base.format('ts'))), ncio.open_dataset(str(outd / base.format('ts')))
        H.same_bits(np.asarray(a['ts'].values), np.asarray(b['ts'].values))
        assert b['ts'].dims == ('time', 'rlat', 'rlon')
