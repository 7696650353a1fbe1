"""tos / siconc onto targets with 2-D coordinates, host side: everything `functions.gauss_interp_points` and the points
branch of `interp_wrapper` decide before the device is touched.  `default_context` is replaced by a function that fails
the test, so each error below is raised - and the empty result returned - with no GPU present."""
import os
import re

import numpy as np
import pytest

from pgw4era5_amd import _lib, functions as F, ncio, synthetic

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pgw_hip.h')


@pytest.fixture(autouse=True)
def no_gpu(monkeypatch):
    def touched():
        raise AssertionError('the context was touched')
    monkeypatch.setattr(F, 'default_context', touched)


def _source():
    oc = synthetic.make_ocean_grid_case(nj=6, ni=8, ntime=12, seed=0, land_patches=1)
    return oc


def _origin(oc, ntime=12, var='tos'):
    ds = ncio.Dataset()
    ds['time'] = ncio.Field(oc['times'][:ntime], ('time',))
    ds['latitude'] = ncio.Field(oc['latitude'], ('j', 'i'))
    ds['longitude'] = ncio.Field(oc['longitude'], ('j', 'i'))
    ds[var] = ncio.Field(oc['values'][:ntime], ('time', 'j', 'i'), attrs={'units': 'K'})
    return ds


def _target(lat, lon, dims_lat, dims_lon, land, land_dims):
    ds = ncio.Dataset()
    ds['lat'] = ncio.Field(np.asarray(lat), dims_lat)
    ds['lon'] = ncio.Field(np.asarray(lon), dims_lon)
    ds['FR_LAND'] = ncio.Field(np.asarray(land), land_dims)
    return ds


def test_target_shapes_are_checked_first():
    oc = _source()
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(5, 7)
    fields = list(oc['values'])
    with pytest.raises(ValueError) as e:
        F.gauss_interp_points(None, lat2, lon2[:, :6], oc['latitude'], oc['longitude'], fields, 1e6, 4.0)
    assert str(e.value) == 'target latitudes of shape (5, 7) and longitudes of shape (5, 6) must have one common shape of rank >= 1'
    with pytest.raises(ValueError, match='rank >= 1'):
        F.gauss_interp_points(None, 45.0, 10.0, oc['latitude'], oc['longitude'], fields, 1e6, 4.0)
    with pytest.raises(ValueError) as e:
        F.gauss_interp_points(np.zeros((7, 5)), lat2, lon2, oc['latitude'], oc['longitude'], fields, 1e6, 4.0)
    assert str(e.value) == 'land fraction of shape (7, 5) does not lie on the targets of shape (5, 7)'
    with pytest.raises(ValueError) as e:
        F.gauss_interp_points(None, lat2, lon2, oc['latitude'], oc['longitude'][:, :7], fields, 1e6, 4.0)
    assert str(e.value) == 'ocean-grid coordinates and values must have the same number of points'


def test_no_targets_give_an_empty_array():
    oc = _source()
    for shape in ((0,), (0, 7), (3, 0)):
        got = F.gauss_interp_points(np.zeros(shape), np.zeros(shape), np.zeros(shape), oc['latitude'], oc['longitude'],
                                    list(oc['values'][:5]), 1e6, 4.0)
        assert got.shape == (5,) + shape and got.dtype == np.float64
    assert F.gauss_interp_points(None, np.zeros(0), np.zeros(0), oc['latitude'], oc['longitude'], [oc['values'][0]], 1e6, 4.0).shape == (1, 0)


def test_interp_wrapper_rejects_a_target_that_is_neither_mesh_nor_points():
    oc = _source()
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(5, 7)
    for tgt in (_target(lat2, lon2[:, :6], ('rlat', 'rlon'), ('rlat', 'rlon2'), np.zeros((5, 7)), ('rlat', 'rlon')),
                _target(lat2, lon2.T, ('rlat', 'rlon'), ('rlon', 'rlat'), np.zeros((5, 7)), ('rlat', 'rlon')),
                _target(lat2, lon2[0], ('rlat', 'rlon'), ('rlon',), np.zeros((5, 7)), ('rlat', 'rlon'))):
        with pytest.raises(ValueError) as e:
            F.interp_wrapper(_origin(oc), tgt, 'tos')
        with pytest.raises(ValueError) as e2:                      # regrid_lat_lon's own text for the same target
            F.regrid_lat_lon(ncio.Dataset(variables={'lat': ncio.Field(np.arange(3.0), ('lat',)),
                                                     'lon': ncio.Field(np.arange(4.0), ('lon',))}), tgt, 'ta')
        assert str(e.value) == str(e2.value)
        assert re.search(r'neither two 1-D axes of a mesh nor point-wise coordinates over the same dimensions$', str(e.value))
        assert '(5, 7)' in str(e.value)


def test_interp_wrapper_rejects_a_land_fraction_of_another_shape():
    oc = _source()
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(5, 7)
    for land, dims in ((np.zeros((2, 5, 7)), ('time', 'rlat', 'rlon')), (np.zeros((7, 5)), ('rlon', 'rlat')),
                       (np.zeros((1, 1, 5, 7)), ('time', 'z', 'rlat', 'rlon')), (np.zeros(35), ('cell',))):
        tgt = _target(lat2, lon2, ('rlat', 'rlon'), ('rlat', 'rlon'), land, dims)
        with pytest.raises(ValueError) as e:
            F.interp_wrapper(_origin(oc, var='siconc'), tgt, 'siconc')
        assert str(land.shape) in str(e.value) and '(5, 7)' in str(e.value) and str(e.value).startswith('FR_LAND of shape')


@pytest.mark.parametrize('land_shape,land_dims', [((5, 7), ('rlat', 'rlon')), ((1, 5, 7), ('time', 'rlat', 'rlon'))])
def test_interp_wrapper_keeps_the_twelve_months_rule(land_shape, land_dims):
    oc = _source()
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(5, 7)
    tgt = _target(lat2, lon2, ('rlat', 'rlon'), ('rlat', 'rlon'), np.zeros(land_shape), land_dims)
    with pytest.raises(ValueError) as e:
        F.interp_wrapper(_origin(oc, ntime=11), tgt, 'tos')
    assert str(e.value) == 'could not broadcast input array: tos has 11 time steps, the ocean-grid interpolation expects 12 months'


def test_nan_ignoring_interp_applies_the_rule_to_labelled_coordinates():
    oc = _source()
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(5, 7)
    delta = ncio.Field(oc['values'][0], ('j', 'i'), {'latitude': oc['latitude'], 'longitude': oc['longitude']})
    land = ncio.Field(np.zeros((5, 7)), ('rlat', 'rlon'), {'lat': lat2, 'lon': lon2[:, :6]})
    with pytest.raises(ValueError, match='neither two 1-D axes of a mesh nor point-wise coordinates'):
        F.nan_ignoring_interp(land, delta, 1e6, 4.0)


def test_the_two_entries_are_declared_and_bound():
    hdr = open(HEADER).read()
    assert _lib.SIGNATURES['pgw_ocean_targets'] == (_lib._i, [_lib._vp, _lib._ll] + [_lib._vp] * 5)
    assert _lib.SIGNATURES['pgw_gauss_interp_points'] == _lib.SIGNATURES['pgw_gauss_interp']
    assert re.search(r'\bint pgw_ocean_targets\(pgw_ctx \*ctx, long long n, const double \*lat, const double \*lon, '
                     r'const double \*land, double \*tx,\s+double \*ty\);', hdr)
    a = re.search(r'\bint pgw_gauss_interp\(([^;]*)\);', hdr).group(1)
    b = re.search(r'\bint pgw_gauss_interp_points\(([^;]*)\);', hdr).group(1)
    assert ' '.join(a.split()) == ' '.join(b.split())              # the same arguments under its own name
