"""Winds of a rotated-pole source grid through the curvilinear regridding, the parts that need no GPU: the C-ABI declaration,
the `--source_winds` flag of step_02 and everything it refuses before a file is written, and the numpy statement of the
definition (source_winds_cases.statement) on a flow with a known answer."""
import os

import numpy as np
import pytest

import source_winds_cases as S
import test_regrid_curvilinear_host as H
import wind_rotation_cases as W
from pgw4era5_amd import _lib, ncio, settings
from pgw4era5_amd import step_02_preproc_deltas as s2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the library and the parser
def test_the_library_exports_the_entry():
    lib = _lib.load()
    assert len(_lib.SIGNATURES['pgw_regrid_sparse_wind'][1]) == 17 and lib.pgw_regrid_sparse_wind is not None
    header = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    assert 'int pgw_regrid_sparse_wind(pgw_ctx *ctx' in header


def test_parsing_the_flag():
    p = s2.parser()
    base = ['regridding', '-i', 'a', '-o', 'b', '-e', 'c']
    assert p.parse_args(base).source_winds is None and p.parse_args(base).rotate_winds is None
    assert p.parse_args(base + ['--source_winds']).source_winds == 'auto'
    assert p.parse_args(['regridding', '--source_winds', '-i', 'a']).source_winds == 'auto'
    assert p.parse_args(base + ['--source_winds', '39.25,-162']).source_winds == '39.25,-162'
    assert p.parse_args(base + ['--source_winds=-30,20']).source_winds == '-30,20'
    assert p.parse_args(base + ['--source_winds', 'geographic', '--rotate_winds']).source_winds == 'geographic'
    assert p.parse_args(base + ['--source_winds', '--rotate_winds']).rotate_winds == 'auto'


# ------------------------------------------------------------------ what the command line refuses
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('source_winds'))
    shape = dict(nrlat=6, nrlon=8, nplev=2, ntime=2)
    latlon = os.path.join(tmp, 'gcm_latlon')                              # sources with 1-D lat / lon axes
    W.write_sources(latlon)
    return dict(tmp=tmp, shape=shape, gcm=S.write_sources(os.path.join(tmp, 'gcm'), **shape), latlon=latlon,
                mesh=S.write_mesh_target(os.path.join(tmp, 'mesh.nc')), rotated=S.write_rotated_target(os.path.join(tmp, 'rotated.nc')))


@pytest.fixture
def xesmf(monkeypatch):
    monkeypatch.setattr(settings, 'i_use_xesmf_regridding', 1)


def refused(files, name, match, gcm=None, target=None, variables='ua,va,ta', flag=('--source_winds',), step='regridding'):
    out = os.path.join(files['tmp'], 'out_' + name)
    argv = [step, '-i', gcm or files['gcm'], '-o', out, '-e', target or files['mesh'], '-v', variables] + list(flag)
    with pytest.raises(ValueError, match=match):
        s2.main(argv)
    assert not os.path.exists(out) or os.listdir(out) == []


def test_refused_with_smoothing(files, xesmf):
    refused(files, 'smoothing', 'belongs to the regridding step', step='smoothing')


def test_refused_in_the_default_branch(files):
    assert settings.i_use_xesmf_regridding == 0
    refused(files, 'default_branch', 'needs settings.i_use_xesmf_regridding = 1', gcm=files['latlon'])
    refused(files, 'default_branch_rot', 'needs settings.i_use_xesmf_regridding = 1', gcm=files['latlon'], target=files['rotated'],
            flag=('--source_winds', 'geographic', '--rotate_winds'))


def test_rotate_winds_alone_is_still_refused_with_the_setting_on(files, xesmf):
    refused(files, 'rotate_alone', 'i_use_xesmf_regridding = 1 is not built', target=files['rotated'], flag=('--rotate_winds',))


def test_refused_for_one_wind_component_without_the_other(files, xesmf):
    refused(files, 'ua_only', 'ua without va', variables='ua,ta')
    refused(files, 'va_only', 'va without ua', variables='ta,va')
    refused(files, 'neither', 'needs ua and va together', variables='ta')


def test_refused_for_a_pole_on_1d_source_coordinates(files, xesmf):
    refused(files, 'pole_1d', '2-D source coordinates', gcm=files['latlon'], flag=('--source_winds', '39.25,-162'))


def test_refused_for_geographic_without_rotate_winds(files, xesmf):
    refused(files, 'geographic', 'nothing to rotate', flag=('--source_winds', 'geographic'))


def test_refused_for_a_pole_that_is_no_position(files, xesmf):
    for text in ('39.25', '39.25,-162,3', 'north,-162', '91,0'):
        refused(files, 'pole', '--source_winds( takes|: a pole)', flag=('--source_winds', text))


def test_refused_when_auto_finds_no_mapping(files, xesmf):
    bare = S.write_sources(os.path.join(files['tmp'], 'gcm_bare'), variables=('ua', 'va'), mapping=False, **files['shape'])
    refused(files, 'no_mapping', '--source_winds auto: no rotated mapping found - the source ua file', gcm=bare, variables='ua,va')


def test_refused_on_a_mesh_target_with_rotate_winds(files, xesmf):
    refused(files, 'mesh_rotate', 'geographic already', flag=('--source_winds', '--rotate_winds', '43,-170'))


def test_refused_when_the_two_files_differ(files, xesmf):
    def float64_va(var, ds):
        if var == 'va':
            ds['va'] = ncio.Field(ds['va'].values.astype(np.float64), ds['va'].dims, ds['va'].coords, ds['va'].attrs)

    def other_lon(var, ds):
        if var == 'va':
            ds['lon'] = ncio.Field(ds['lon'].values + 0.5, ds['lon'].dims)

    for name, edit, match in (('dtype', float64_va, '--source_winds: ua and va differ in dtype'),
                              ('grid', other_lon, '--source_winds: ua and va differ in their source grid')):
        path = S.write_sources(os.path.join(files['tmp'], 'gcm_' + name), variables=('ua', 'va'), edit=edit, **files['shape'])
        refused(files, name, match, gcm=path, variables='ua,va')
    only_ua = S.write_sources(os.path.join(files['tmp'], 'gcm_only_ua'), variables=('ua',), **files['shape'])
    refused(files, 'missing', 'Files for variable va are missing', gcm=only_ua, variables='ua,va')


# ------------------------------------------------------------------ the statement
def test_statement_turns_the_solid_body_flow_to_geographic():
    """Grid-relative (cos rlat, 0) on the rot24x48 grid is the solid-body flow about the grid's pole.  The statement fed with it
    must give what the weights give for the analytic geographic components, to 1e-13: the bound
    test_solid_body_rotation_has_no_grid_northward_component grants the rotation of a unit wind, which convex weights
    (non-negative, summing to 1 to rounding) do not enlarge.  Without the source rotation it must be off by more than 0.05:
    the grid's directions are up to 33 degrees off geographic."""
    case = S.solid_body_case()
    idx, w, n_un, _ = H.locate_statement(case['X'], case['P'], False)
    assert n_un == 0
    want = [H.apply_statement(g, idx, w) for g in case['geo']]
    got = S.statement(*case['grid'], idx, w, src=case['src'])
    plain = S.statement(*case['grid'], idx, w)
    err = max(np.abs(g - x).max() for g, x in zip(got, want))
    off = max(np.abs(g - x).max() for g, x in zip(plain, want))
    print('solid body: |statement - analytic| = %.3e, without the source rotation %.3f' % (err, off))
    assert err <= 1e-13 and off > 0.05


def test_statement_order_rounding_and_pairs():
    """A self-check of the checker on a case small enough to follow: float32 values are rounded after the source rotation and
    after the weights; a target rotation acts on an unmapped target's 0.0; both pairs None is apply_statement per component."""
    rng = np.random.default_rng(1)
    ua, va = rng.standard_normal((2, 3, 4)).astype(np.float32), rng.standard_normal((2, 3, 4)).astype(np.float32)
    idx = np.array([[0, 1, 5, 4], [-1, -1, -1, -1], [6, 7, 11, 10]], dtype=np.int32)
    w = np.array([[0.25, 0.25, 0.25, 0.25], [0, 0, 0, 0], [0.5, 0.125, 0.125, 0.25]])
    src, targ = S.angles((3, 4), 2), S.angles((3,), 3)
    u, v = S.statement(ua, va, idx, w)
    np.testing.assert_array_equal(u, H.apply_statement(ua, idx, w))
    np.testing.assert_array_equal(v, H.apply_statement(va, idx, w))
    ug, vg = W.rotate(ua, va, *src, inverse=True)
    assert ug.dtype == np.float32
    ur, vr = H.apply_statement(ug, idx, w), H.apply_statement(vg, idx, w)
    for got, want in zip(S.statement(ua, va, idx, w, src, targ), W.rotate(ur, vr, *targ)):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)
    assert (np.asarray(S.statement(ua, va, idx, w, src, targ))[:, :, 1] == 0.0).all()
    assert np.isnan(np.asarray(S.statement(ua, va, idx, w, src, targ, unmapped_nan=True))[:, :, 1]).all()
    assert S.statement(ua, va.astype(np.float64), idx, w, src)[0].dtype == np.float64
