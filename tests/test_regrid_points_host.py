"""Regridding onto point-wise targets in the default branch (`pgw_regrid_points`: k_regrid_points; `functions.regrid_points`,
`functions.regrid_lat_lon` with 2-D target coordinates): the statement of correctness, the case builders and the host tests
that keep both honest.  tests/test_regrid_points_hip.py imports everything from here.  No GPU is needed in this file.

`statement` is the definition: per target g and plane, in float64 on the stored values, on the tables
`functions.regrid_tables(src_lat, src_lon, targ_lat.ravel(), targ_lon.ravel())` yields,
    ya = (v[hi_row, lon_lo] - v[lo_row, lon_lo]) / lat_Dx * lat_dx + v[lo_row, lon_lo]
    yb = the same at lon_hi;      out = (yb - ya) / lon_Dx * lon_dx + ya
stored in the field's dtype; row -1 / nlat_s is the pole value (numpy's nanmean here, k_zonal_mean_rows on the GPU),
`lat_oob | lon_oob` gives NaN.  It is tied (1) to `scipy.interpolate.interp1d` applied latitude first, then longitude point
by point - what xarray's `.interp({lat: targ_lat}).interp({lon: targ_lon})` does with coordinates over shared dimensions
(reference functions.py:859, :892) - bit for bit on rotated-pole targets, and (2) to the separable computation of k_regrid
(`kernel_statement` of tests/test_regrid_edges_host.py) bit for bit on a mesh handed over as points.  PARITY WITH XARRAY
ITSELF IS UNPINNED (not importable here).

Every case builder asserts the condition that makes its case what its name says."""
import functools

import numpy as np
import pytest
from scipy.interpolate import interp1d

import test_regrid_edges_host as E                                                  # noqa: E402
from function_recorder import RecordingContext
from pgw4era5_amd import device, ncio, synthetic
from pgw4era5_amd import functions as F

BLOCK = 256                        # threads per block of k_regrid_points


# ------------------------------------------------------------------ the statement
def _div(n, d):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(d == 0, np.nan, n / np.where(d == 0, 1.0, d))


def numpy_poles(field, tb):
    """(nfield, 2) south / north pole values: numpy's NaN-skipping mean of the rows the tables name (NaN where none)."""
    f = np.asarray(field)
    f = f.reshape((-1,) + f.shape[-2:]).astype(np.float64)
    p = np.full((f.shape[0], 2), np.nan)
    for k, r in enumerate((tb['south_row'], tb['north_row'])):
        if r >= 0:
            ok = ~np.isnan(f[:, r, :])
            n = ok.sum(axis=1)
            with np.errstate(invalid='ignore', divide='ignore'):
                p[:, k] = np.where(n > 0, np.where(ok, f[:, r, :], 0.0).sum(axis=1) / np.maximum(n, 1), np.nan)
    return p


def touches_pole(tb, nlat_s):
    """(ntarg,) bool: targets whose latitude bracket names a pole row."""
    return (tb['lat_lo'] < 0) | (tb['lat_lo'] >= nlat_s) | (tb['lat_hi'] < 0) | (tb['lat_hi'] >= nlat_s)


def statement(field, tb, pole=None):
    """field (..., nlat_s, nlon_s), per-point tables `tb` -> (nfield, ntarg) in the field's dtype."""
    field = np.asarray(field)
    nlat_s, nlon_s = field.shape[-2:]
    f = field.reshape(-1, nlat_s, nlon_s).astype(np.float64)
    pole = numpy_poles(field, tb) if pole is None else pole

    def v(rows, cols):
        inner = f[:, rows.clip(0, nlat_s - 1), cols]
        return np.where(rows[None] < 0, pole[:, 0:1], np.where(rows[None] >= nlat_s, pole[:, 1:2], inner))
    jl, jh, il, ih = tb['lat_lo'], tb['lat_hi'], tb['lon_lo'], tb['lon_hi']
    with np.errstate(invalid='ignore'):
        ya = _div(v(jh, il) - v(jl, il), tb['lat_Dx'][None]) * tb['lat_dx'][None] + v(jl, il)      # lat pass at the lower column
        yb = _div(v(jh, ih) - v(jl, ih), tb['lat_Dx'][None]) * tb['lat_dx'][None] + v(jl, ih)      # ... at the upper column
        out = _div(yb - ya, tb['lon_Dx'][None]) * tb['lon_dx'][None] + ya                          # lon pass
    out[:, (tb['lat_oob'] | tb['lon_oob']) != 0] = np.nan
    return np.ascontiguousarray(out.astype(field.dtype))          # C order: numpy's own reductions depend on the layout


def tables(slat, slon, tlat, tlon):
    return F.regrid_tables(slat, slon, np.asarray(tlat, dtype=np.float64).ravel(), np.asarray(tlon, dtype=np.float64).ravel())


def interp1d_composition(field, slat, slon, tlat, tlon):
    """scipy's interp1d along latitude at every target latitude, then along longitude point by point, on the dataset the
    reference has formed by then (flip, +-360 copies); for cases without pole rows.  -> (nfield, ntarg) float64."""
    f = np.asarray(field)
    f = f.reshape((-1,) + f.shape[-2:]).astype(np.float64)
    slat, slon = np.asarray(slat, dtype=np.float64), np.asarray(slon, dtype=np.float64)
    tlat, tlon = np.asarray(tlat, dtype=np.float64).ravel(), np.asarray(tlon, dtype=np.float64).ravel()
    periodic = (np.median(np.diff(slon)) + slon.max() - slon.min()) >= 359.9
    if slat[0] > slat[-1]:
        slat, f = slat[::-1], f[:, ::-1, :]
    y = interp1d(slat, f, axis=1, bounds_error=False)(tlat)                          # (nfield, ntarg, nlon_s)   :859
    lon = slon
    if periodic:                                                                      # :866-874
        if tlon.max() > lon.max():
            y, lon = np.concatenate([y, y], axis=-1), np.concatenate([lon, lon + 360])
        if tlon.min() < lon.min():
            y, lon = np.concatenate([y, y], axis=-1), np.concatenate([lon - 360, lon])
    out = np.empty((f.shape[0], tlat.size))
    for g in range(tlat.size):                                                        # :892, point by point
        out[:, g] = interp1d(lon, y[:, g, :], axis=-1, bounds_error=False)(tlon[g])
    return out


def same_bits(a, b):
    """dtype, shape, NaN mask and the bits of every other value equal (which NaN an operation on a NaN produces - sign and
    payload - is left open, as IEEE 754 does)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg='NaN mask')
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    ok = ~np.isnan(a)
    np.testing.assert_array_equal(a.view(u)[ok], b.view(u)[ok])


# ------------------------------------------------------------------ the launch rule
def slices(nfield, ntarg):
    """The launch rule of pgw_regrid_points (one target per thread): (gz, planes per slice, planes each slice really has)."""
    bx = -(-ntarg // BLOCK)
    gz = min(max(-(-8192 // bx), 1), nfield, 65535)
    per = -(-nfield // gz)
    return gz, per, [max(0, min(nfield, (z + 1) * per) - z * per) for z in range(gz)]


# ------------------------------------------------------------------ the cases
def _field(rng, shape):
    """Values of both signs, never 0; plane k lies around 100 (k + 1), so a plane taken from the wrong source plane shows."""
    return rng.normal(0.0, 5.0, shape) + 100.0 * (1 + np.arange(shape[0]).reshape(-1, 1, 1))


class Case:
    """field (nfield, nlat_s, nlon_s) float64, source axes, flat targets; tables and pole mask."""

    def __init__(self, field, slat, slon, tlat, tlon):
        self.field = np.ascontiguousarray(field, dtype=np.float64)
        self.slat, self.slon = np.asarray(slat, dtype=np.float64), np.asarray(slon, dtype=np.float64)
        self.tlat, self.tlon = np.asarray(tlat, dtype=np.float64), np.asarray(tlon, dtype=np.float64)
        assert self.tlat.shape == self.tlon.shape
        self.nfield, self.nlat_s, self.nlon_s = self.field.shape
        self.ntarg = self.tlat.size
        self.tb = tables(self.slat, self.slon, self.tlat, self.tlon)
        self.pole = touches_pole(self.tb, self.nlat_s)

    def want(self, dtype):
        return statement(self.field.astype(dtype), self.tb)


def source(kind, nlat_s, nlon_s):
    """Source axes: 'asc0' ascending latitudes, longitudes 0 ... 360; 'desc180' descending, -180 ... 180; 'regional' a
    non-periodic box around the rotated grid of synthetic.rotated_pole_grid."""
    x = (np.arange(nlat_s) + 0.5) / nlat_s
    lat = (-90.0 + 180.0 * x) * (1 - 0.3 / nlat_s)
    lon = np.arange(nlon_s) * (360.0 / nlon_s)
    if kind == 'desc180':
        lat, lon = lat[::-1].copy(), lon - 180.0
    elif kind == 'regional':
        lat, lon = np.linspace(20.0, 75.0, nlat_s), np.linspace(-50.0, 70.0, nlon_s)
    elif kind != 'asc0':
        raise KeyError(kind)
    return lat, lon


@functools.lru_cache(maxsize=None)
def rotated_case(kind, nlat_s, nlon_s, ntarg, nfield=3):
    """The leading `ntarg` points of a 24 x 48 rotated-pole grid: no target brackets a pole row."""
    slat, slon = source(kind, nlat_s, nlon_s)
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(24, 48)
    c = Case(_field(np.random.default_rng(nlat_s + ntarg), (nfield, nlat_s, nlon_s)), slat, slon, lat2.ravel()[:ntarg], lon2.ravel()[:ntarg])
    assert c.tb['south_row'] == c.tb['north_row'] == -1 and not c.pole.any()         # no target brackets a pole row
    assert c.tb['periodic'] == (kind != 'regional') and not (c.tb['lat_oob'] | c.tb['lon_oob']).any()
    return c


@functools.lru_cache(maxsize=None)
def random_case(kind, nlat_s, nlon_s, ntarg, nfield=3):
    """A random point list over the whole source (the globe for the periodic kinds: pole rows and both +-360 copies are in
    use), in random order: at most 0.10 of the targets bracket a pole row."""
    rng = np.random.default_rng(7 * nlat_s + ntarg)
    slat, slon = source(kind, nlat_s, nlon_s)
    tlat = rng.uniform(slat.min(), slat.max(), ntarg)
    if kind == 'regional':
        tlon = rng.uniform(slon.min(), slon.max(), ntarg)
    else:
        tlon = rng.uniform(-200.0, 380.0, ntarg) if kind == 'asc0' else rng.uniform(-180.0, 180.0, ntarg)
    if kind == 'asc0' and ntarg >= 63:                            # both poles and a few targets between them and the edge rows
        k = ntarg // 20
        tlat[:k] = np.where(rng.random(k) < 0.5, -1.0, 1.0) * rng.uniform(slat.max(), 90.0, k)
        tlat[:2] = [-90.0, 90.0]
    c = Case(_field(rng, (nfield, nlat_s, nlon_s)), slat, slon, tlat, tlon)
    if ntarg >= 63:
        assert c.pole.mean() <= 0.10, c.pole.mean()
    if ntarg >= 63 and kind != 'regional' and slat[0] < slat[-1]:
        assert c.pole.any() and c.tb['south_row'] >= 0 and c.tb['north_row'] >= 0
    return c


@functools.lru_cache(maxsize=None)
def mesh_case(which):
    """A mesh handed over as points: '37x72' (make_gcm_grid_case) and '7x9' with rows at -90 and 90; pole rows included."""
    if which == '37x72':
        g = synthetic.make_gcm_grid_case(ntime=1, nplev=3, seed=4)
        f, slat, slon, tlat, tlon = g['field'][0], g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon']
    else:
        slat, slon = source('asc0', 12, 20)
        f = _field(np.random.default_rng(79), (3, 12, 20))
        tlat, tlon = np.linspace(-90.0, 90.0, 7), np.linspace(-170.0, 350.0, 9)
    la2, lo2 = np.meshgrid(tlat, tlon, indexing='ij')
    c = Case(f, slat, slon, la2.ravel(), lo2.ravel())
    c.mesh = (tlat, tlon)
    assert c.pole.any() and c.tb['south_row'] >= 0 and c.tb['north_row'] >= 0
    return c


SLAT36, SLON720 = source('asc0', 36, 720)


def _box_targets(r0, c0, nrow, span, n, seed):
    """n targets on the 36 x 720 source whose entries cover exactly rows r0 ... r0 + nrow - 1 and columns c0 ... c0 + span
    - 1 (modulo 720), in random order."""
    rng = np.random.default_rng(seed)
    r = rng.integers(r0, r0 + nrow - 1, n)
    cc = rng.integers(c0, c0 + span - 1, n)
    r[:3], cc[:3] = [r0, r0 + nrow - 2, r0], [c0, c0 + span - 2, c0 + span - 2]
    tlat = SLAT36[r] + rng.uniform(0.2, 0.8, n) * (SLAT36[r + 1] - SLAT36[r])
    tlon = (cc + rng.uniform(0.2, 0.8, n)) * 0.5
    return tlat, tlon


@functools.lru_cache(maxsize=None)
def layout_case(name):
    """Blocks of targets laid out as the name says, the condition asserted from the tables."""
    rng = np.random.default_rng(len(name))
    f = _field(rng, (3, 36, 720))
    if name == 'seam':                                                                # two blocks across the periodic seam
        tlat, tlon = _box_targets(5, 700, 4, 40, 512, seed=1)
        c = Case(f, SLAT36, SLON720, tlat, np.where(tlon >= 360.0, tlon - 360.0, tlon))
        assert (c.tb['lon_lo'] == 719).any() and (c.tb['lon_hi'] == 0).any()          # a target in the gap itself
        assert (c.tb['lon_lo'] >= 700).any() and (c.tb['lon_hi'] <= 19).any() and not c.pole.any()
    elif name == 'both poles':                                                        # one block holding both poles
        tlat = np.concatenate([[-90.0, 90.0, -89.9, 89.9], np.linspace(-88.0, 88.0, 252)])
        c = Case(f, SLAT36, SLON720, tlat, np.linspace(100.0, 300.0, 256))
        assert c.pole[:4].all() and (c.tb['lat_lo'][:4] == [-1, 35, -1, 35]).all() and (c.tb['lat_hi'][:4] == [0, 36, 0, 36]).all()
    elif name == 'poles only':                                                        # every bracket of a block names the north pole row
        c = Case(f, SLAT36, SLON720, np.full(64, 89.95), np.linspace(100.0, 104.0, 64))
        assert c.pole.all() and c.tb['north_row'] == 35 and (c.tb['lat_hi'] == 36).all()
    elif name == 'random order':                                                      # 1030 targets all over the source
        tlat, tlon = _box_targets(0, 0, 36, 720, 1030, seed=3)
        c = Case(f, SLAT36, SLON720, tlat, tlon)
        assert np.ptp(c.tb['lat_lo'][:256]) > 30 and np.ptp(c.tb['lon_lo'][:256]) > 700
    elif name == 'neighbours':                                                        # 1029 neighbouring targets: five blocks, the last one ragged
        tlat, tlon = _box_targets(7, 300, 5, 30, 1029, seed=4)
        c = Case(f, SLAT36, SLON720, tlat, tlon)
        assert 4 * BLOCK < c.ntarg < 5 * BLOCK and np.ptp(c.tb['lat_lo']) == 3 and np.ptp(c.tb['lon_lo']) == 28
    else:
        raise KeyError(name)
    return c


LAYOUT_CASES = ['seam', 'both poles', 'poles only', 'random order', 'neighbours']


# ------------------------------------------------------------------ host tests: the statement
def test_statement_equals_interp1d_composition_on_rotated_targets():
    """All 1152 x 3 values equal, none NaN; the same with descending latitudes / longitudes from -180 and a regional source."""
    for kind in ('asc0', 'desc180', 'regional'):
        c = rotated_case(kind, 48, 96, 1152)
        got = c.want(np.float64)
        assert not np.isnan(got).any()
        same_bits(got, interp1d_composition(c.field, c.slat, c.slon, c.tlat, c.tlon))


@pytest.mark.parametrize('which', ['37x72', '7x9'])
def test_statement_equals_the_separable_computation_on_a_mesh(which):
    c = mesh_case(which)
    tlat, tlon = c.mesh
    tb = F.regrid_tables(c.slat, c.slon, tlat, tlon)
    pole = numpy_poles(c.field, tb)
    want = E.kernel_statement(c.field, tb, pole).reshape(c.nfield, -1)
    assert (c.tb['south_row'], c.tb['north_row']) == (tb['south_row'], tb['north_row'])
    same_bits(statement(c.field, c.tb, pole), want)
    same_bits(statement(c.field.astype(np.float32), c.tb, pole), E.kernel_statement(c.field.astype(np.float32), tb, pole).reshape(c.nfield, -1))


@pytest.mark.parametrize('name', LAYOUT_CASES)
def test_layout_case_conditions(name):
    c = layout_case(name)
    assert c.want(np.float32).shape == (3, c.ntarg)


def test_case_builders_and_helpers():
    for kind, ns in (('asc0', (5, 8)), ('desc180', (48, 96)), ('regional', (48, 96))):
        for n in (1, 63, 513, 1030):
            c = random_case(kind, ns[0], ns[1], n)
            assert c.ntarg == n
    assert slices(40, 1030) == (40, 1, [1] * 40) and slices(3, 512)[0] == 3 and slices(228, 1038240) == (3, 76, [76, 76, 76])


# ------------------------------------------------------------------ host tests: the Python layer on the recording stand-in
def _gcm(lat, lon, dtype=np.float32):
    ds = ncio.Dataset(attrs=dict(title='t'))
    times = np.array(['1995-%02d-15T12:00:00' % (m + 1) for m in range(2)], dtype='datetime64[s]')
    plev = np.array([85000.0, 50000.0])
    ds['time'] = ncio.Field(times, ('time',))
    ds['plev'] = ncio.Field(plev, ('plev',), attrs=dict(units='Pa'))
    ds['lat'] = ncio.Field(lat, ('lat',), attrs=dict(units='degrees_north'))
    ds['lon'] = ncio.Field(lon, ('lon',), attrs=dict(units='degrees_east'))
    ds['ta'] = ncio.Field(np.ones((2, 2, len(lat), len(lon)), dtype), ('time', 'plev', 'lat', 'lon'), {'time': times, 'plev': plev},
                          dict(units='K'))
    ds['ts'] = ncio.Field(np.ones((2, len(lat), len(lon)), dtype), ('time', 'lat', 'lon'), {'time': times}, dict(units='K'))
    ds['time_bnds'] = ncio.Field(np.zeros((2, 2)), ('time', 'bnds'))
    return ds


def _target(lat, lon, dims_lat, dims_lon):
    ds = ncio.Dataset()
    ds['lat'] = ncio.Field(np.asarray(lat), dims_lat)
    ds['lon'] = ncio.Field(np.asarray(lon), dims_lon)
    return ds


@pytest.fixture
def rec(monkeypatch):
    ctx = RecordingContext()
    monkeypatch.setattr(F, 'default_context', lambda: ctx)
    monkeypatch.setattr(device, 'default_context', lambda: ctx)
    return ctx


def test_2d_target_issues_one_points_call_per_horizontal_variable(rec):
    slat, slon = source('asc0', 24, 48)
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(7, 9)
    out = F.regrid_lat_lon(_gcm(slat, slon), _target(lat2, lon2, ('rlat', 'rlon'), ('rlat', 'rlon')), 'ta')
    assert rec.entries() == ['pgw_regrid_points', 'pgw_regrid_points']
    (_, a), (_, b) = rec.calls
    assert a[2:6] == (4, 24, 48, 63) and b[2:6] == (2, 24, 48, 63)                  # nfield, nlat_s, nlon_s, ntarg
    assert out['ta'].dims == ('time', 'plev', 'rlat', 'rlon') and out['ta'].shape == (2, 2, 7, 9) and out['ta'].dtype == np.float32
    assert out['ts'].dims == ('time', 'rlat', 'rlon') and out['ta'].attrs == dict(units='K')
    assert out['lat'].dims == out['lon'].dims == ('rlat', 'rlon') and out['lat'].attrs == dict(units='degrees_north')
    np.testing.assert_array_equal(out['lat'].values, lat2)
    np.testing.assert_array_equal(out['lon'].values, lon2)
    assert 'time_bnds' in out and 'plev' in out and out.attrs == dict(title='t')
    # an unstructured cell list: 1-D lat / lon over one shared dimension
    rec.calls.clear()
    o = F.regrid_lat_lon(_gcm(slat, slon), _target(lat2.ravel(), lon2.ravel(), ('cell',), ('cell',)), 'ts')
    assert rec.entries() == ['pgw_regrid_points'] * 2 and o['ts'].dims == ('time', 'cell') and o['lat'].dims == ('cell',)


def test_mesh_target_stays_on_the_separable_entry(rec):
    slat, slon = source('asc0', 24, 48)
    out = F.regrid_lat_lon(_gcm(slat, slon), _target(np.linspace(30.0, 60.0, 7), np.linspace(-10.0, 30.0, 9), ('lat',), ('lon',)), 'ta')
    assert rec.entries() == ['pgw_regrid_bilinear', 'pgw_regrid_bilinear']
    assert out['ta'].dims == ('time', 'plev', 'lat', 'lon') and out['lat'].dims == ('lat',)


def test_mismatched_target_shapes_raise_before_any_call(rec):
    slat, slon = source('asc0', 24, 48)
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(7, 9)
    for tgt in (_target(lat2, lon2[:, :8], ('rlat', 'rlon'), ('rlat', 'rlon2')),
                _target(lat2, lon2.T, ('rlat', 'rlon'), ('rlon', 'rlat')),
                _target(lat2, lon2[0], ('rlat', 'rlon'), ('rlon',))):
        with pytest.raises(ValueError, match=r'\(7, 9\)'):
            F.regrid_lat_lon(_gcm(slat, slon), tgt, 'ta')
    with pytest.raises(ValueError, match='common shape'):
        F.regrid_points(np.ones((24, 48)), slat, slon, lat2, lon2[:, :8])
    with pytest.raises(ValueError, match='source coordinates'):
        F.regrid_points(np.ones((24, 47)), slat, slon, lat2, lon2)
    assert rec.calls == [] and rec.uploads == []


def test_extent_errors_with_a_regional_source(rec):
    slat, slon = source('regional', 24, 48)
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(7, 9)
    assert lat2.min() > slat.min() and lat2.max() < slat.max() and lon2.min() > slon.min() and lon2.max() < slon.max()
    F.regrid_lat_lon(_gcm(slat, slon), _target(lat2, lon2, ('y', 'x'), ('y', 'x')), 'ts')
    n = len(rec.calls)
    for dlat, dlon, word in ((40.0, 0.0, 'North or South'), (-40.0, 0.0, 'North or South'), (0.0, 60.0, 'East or West'),
                             (0.0, -60.0, 'East or West')):
        with pytest.raises(ValueError, match=word):
            F.regrid_lat_lon(_gcm(slat, slon), _target(lat2 + dlat, lon2 + dlon, ('y', 'x'), ('y', 'x')), 'ts')
    assert len(rec.calls) == n
