"""Bilinear regridding from curvilinear / rotated source grids on the GPU (k_cell_locate, k_row_mean_plain, k_regrid_sparse;
regrid_lat_lon's xESMF branch, reference functions.py:797-810).  PARITY WITH ESMF IS UNPINNED (xESMF / ESMF cannot be
imported); the definition written above k_cell_locate in pgw4era5_amd/csrc/pgw_kernels.h is the definition of correctness,
and its numpy statement is tests/test_regrid_curvilinear_host.py (`locate_statement`, `apply_statement`: every cell tried
by brute force).  Here: (1) ground truth by construction, (2) the kernels against the statement bit for bit, (3) the apply
kernel in both of its forms, (4) properties, (5) the drop-in path through regrid_lat_lon and the step_02 command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_regrid_curvilinear_host as H                                              # noqa: E402
from pgw4era5_amd import _lib, functions as F, ncio, settings, synthetic
from pgw4era5_amd.device import default_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def locate(X, P, periodic):
    wts = F.locate_points(X, P, periodic)
    return wts, wts.idx.numpy(), wts.w.numpy()


def sparse(src, wts, direct=False):
    """regrid_curvilinear on (nfield, ny, nx) with the apply form chosen: LDS-staged where the window fits (default), or
    every block gathering directly."""
    ctx = default_context()
    old = ctx.set_option('sparse_direct', 1 if direct else 0)
    try:
        return F.regrid_curvilinear(src, wts)
    finally:
        ctx.set_option('sparse_direct', old)


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


# ----------------------------------------------------------------------------------------------- 1. ground truth
@pytest.mark.parametrize('name', ['2x2', '3x4', '5x7', '5x7p', 'rot24x48'])
@pytest.mark.parametrize('nt', [1, 65, 257])
def test_ground_truth_by_construction(name, nt):
    X, periodic = H.GRIDS[name]()
    P, cell, st = H.truth_targets(X, periodic, nt, seed=100 + nt)
    wts, idx, w = locate(X, P, periodic)
    assert wts.n_unmapped == 0
    H.check_truth(X, periodic, idx, w, cell, st)


def test_ground_truth_cap_triangles():
    X, periodic = H.GRIDS['5x7p']()
    P, cell, st = H.truth_targets(X, periodic, 257, seed=5)
    caps = cell >= 4 * 7
    assert caps.sum() >= 14
    wts, idx, w = locate(X, P[caps], periodic)
    assert wts.n_unmapped == 0 and (idx[:, 3] == -1).all() and (idx[:, 0] >= 35).all()
    H.check_truth(X, periodic, idx, w, cell[caps], st[caps])


# ----------------------------------------------------------------------------------------------- 2. restatement
def special_targets(X, periodic, seed):
    """Ground-truth targets plus the ties and the misses: every node, the midpoints of the cell edges in both directions,
    points outside the grid, a NaN target."""
    def thin(a, n=48):                                            # the brute-force statement is (targets x cells): keep it small
        return a[::max(1, len(a) // n)]
    P, _, _ = H.truth_targets(X, periodic, 65, seed)
    nodes = thin(X.reshape(-1, 3))
    mid_i = thin(H.normalise(0.5 * (X[:, :-1] + X[:, 1:])).reshape(-1, 3))
    mid_j = thin(H.normalise(0.5 * (X[:-1] + X[1:])).reshape(-1, 3))
    rng = np.random.default_rng(seed)
    anywhere = H.normalise(rng.standard_normal((64, 3)))
    nan = np.array([[np.nan, 0.0, 1.0]])
    return np.concatenate([P, nodes, mid_i, mid_j, anywhere, -nodes[:3], nan], axis=0)


def check_restatement(X, periodic, P):
    wts, idx, w = locate(X, P, periodic)
    idx_s, w_s, n_un, _ = H.locate_statement(X, P, periodic)
    np.testing.assert_array_equal(idx, idx_s)
    same_bits(w, w_s)
    assert wts.n_unmapped == n_un
    return n_un


@pytest.mark.parametrize('name', ['2x2', '3x4', '5x7', '5x7p', 'rot24x48'])
def test_locate_equals_statement(name):
    X, periodic = H.GRIDS[name]()
    P = special_targets(X, periodic, seed=21)
    n_un = check_restatement(X, periodic, P)
    if not periodic:
        assert n_un >= 4                                          # the antipodes and the NaN target, at least


def test_nodes_and_edges_go_to_the_lowest_cell():
    X, periodic = H.GRIDS['3x4']()
    P = np.concatenate([X.reshape(-1, 3), H.normalise(0.5 * (X[:, :-1] + X[:, 1:])).reshape(-1, 3)], axis=0)
    _, idx, w = locate(X, P, periodic)
    idx_s, _, _, cell = H.locate_statement(X, P, periodic)
    np.testing.assert_array_equal(idx, idx_s)
    assert cell[1 * 4 + 1] == 0 and cell[1 * 4 + 2] == 1           # inner nodes: four cells accept, the lowest wins
    assert cell[12 + 1 * 3 + 0] == 0                               # midpoint of the edge between cells 0 and 3


@pytest.mark.parametrize('name', ['3x4', '5x7p'])
def test_collapsed_cells_and_nan_coordinates(name):
    X, periodic = H.GRIDS[name]()
    P = special_targets(X, periodic, seed=33)
    Xc = X.copy()
    Xc[1, 2] = Xc[1, 1]                                           # two cells collapse to triangles, none to a point
    Xc[0, 0] = Xc[1, 0] = Xc[0, 1]                                # cell 0 collapses to a line
    check_restatement(Xc, periodic, P)
    Xn = X.copy()
    Xn[1, 1, 0] = np.nan
    n_un = check_restatement(Xn, periodic, P)
    assert n_un > 0


def test_unmapped_count_outside_a_regional_grid():
    X, periodic = H.GRIDS['rot24x48']()
    tlat, tlon = np.meshgrid(np.linspace(20.0, 80.0, 16), np.linspace(-60.0, 90.0, 16), indexing='ij')
    P = F.unit_vectors(tlat, tlon).reshape(-1, 3)
    n_un = check_restatement(X, periodic, P)
    assert 0 < n_un < len(P)


# ----------------------------------------------------------------------------------------------- 3. apply
def field(nf, ny, nx, dtype, seed):
    return np.random.default_rng(seed).standard_normal((nf, ny, nx)).astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('nf', [1, 3, 17])
@pytest.mark.parametrize('name,nt', [('3x4', 1), ('5x7p', 65), ('rot24x48', 257), ('5x7p', 1028)])
def test_apply_equals_statement_in_both_forms(name, nt, nf, dtype):
    """65 / 257 / 1 targets: one value per thread (odd plane length); 1028: 16-byte stores, more than one block."""
    X, periodic = H.GRIDS[name]()
    P = special_targets(X, periodic, seed=nt)
    P = np.concatenate([P] * (nt // len(P) + 1), axis=0)[:nt]
    wts, idx, w = locate(X, P, periodic)
    src = field(nf, X.shape[0], X.shape[1], dtype, seed=nf)
    want = H.apply_statement(src, idx, w)
    staged, direct = sparse(src, wts), sparse(src, wts, direct=True)
    assert staged.dtype == dtype and staged.shape == (nf, nt)
    same_bits(staged, want)
    same_bits(direct, want)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_apply_window_threshold(dtype):
    """A 48 x 96 source plane (4608 elements) is wider than the LDS window: scattered targets make every block gather
    directly on its own, targets sorted along a source row stage their window; same bits as the statement either way."""
    lat, lon = np.meshgrid(np.linspace(-80, 80, 48), np.arange(96) * 3.75, indexing='ij')
    X = F.unit_vectors(lat, lon)
    rng = np.random.default_rng(3)
    scattered = H.normalise(rng.standard_normal((1028, 3)))
    row = F.unit_vectors(np.full(1028, 31.3), np.linspace(1.0, 300.0, 1028))
    src = field(3, 48, 96, dtype, seed=9)
    for P in (scattered, row):
        wts, idx, w = locate(X, P, True)
        want = H.apply_statement(src, idx, w)
        same_bits(sparse(src, wts), want)
        same_bits(sparse(src, wts, direct=True), want)
    inner = idx[(idx >= 0).all(axis=1)]
    assert inner.max() - inner.min() < 2048                        # the row's window fits


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_apply_nan_unmapped_and_absent_entries(dtype, monkeypatch):
    X, periodic = H.GRIDS['5x7p']()
    P = special_targets(X, periodic, seed=4)
    wts, idx, w = locate(X, P, periodic)
    caps = idx[:, 3] == -1
    unmapped = (idx == -1).all(axis=1)
    assert (caps & ~unmapped).any() and unmapped.any()
    src = field(3, 5, 7, dtype, seed=1)
    src[:, 0, 0] = np.nan                      # source element 0: beside every idx = -1 entry, which must stay unread
    src[1, 2, 3] = np.nan
    for direct in (False, True):
        got = sparse(src, wts, direct)
        same_bits(got, H.apply_statement(src, idx, w))
        assert (got[:, unmapped] == 0.0).all()                     # unmapped -> 0.0 like xESMF 0.6.2
        uses_nan = ((idx == 0) | (idx == 35)).any(axis=1)          # node 0 and the pole of row 0, whose mean holds it
        assert np.isnan(got[:, uses_nan]).all() and uses_nan.any()
        clean = ~uses_nan & ~(idx == 2 * 7 + 3).any(axis=1)
        assert not np.isnan(got[:, clean]).any() and (caps & clean).any()
        assert np.isnan(got[1][(idx == 2 * 7 + 3).any(axis=1)]).all()
    monkeypatch.setattr(settings, 'xesmf_unmapped_to_nan', True)
    for direct in (False, True):
        got = sparse(src, wts, direct)
        same_bits(got, H.apply_statement(src, idx, w, unmapped_nan=True))
        assert np.isnan(got[:, unmapped]).all()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_pole_mean_with_and_without_nan(dtype):
    X, periodic = H.GRIDS['5x7p']()
    nodes = H.all_nodes(X, periodic)
    P = nodes[35:37]                                               # the two poles themselves: weight 1 on the pole node
    wts, idx, w = locate(X, P, periodic)
    assert (idx[:, 0] == [35, 36]).all()
    np.testing.assert_allclose(w[:, 0], 1.0, rtol=0, atol=8 * EPS)
    src = field(3, 5, 7, dtype, seed=2)
    src[2, 4, 5] = np.nan                                          # plane 2: a NaN in the last row only
    got = sparse(src, wts)
    same_bits(got, H.apply_statement(src, idx, w))
    means = H.pole_means(src)
    np.testing.assert_allclose(got[:2].astype(np.float64), means[:2], rtol=0,
                               atol=16 * max(EPS, np.finfo(dtype).eps) * np.abs(src[:2]).max())
    assert not np.isnan(got[2, 0]) and np.isnan(got[2, 1])         # the plain mean propagates NaN (no skipping)


# ----------------------------------------------------------------------------------------------- 4. properties
@pytest.mark.parametrize('name', ['5x7p', 'rot24x48'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_constant_in_constant_out(name, dtype):
    X, periodic = H.GRIDS[name]()
    P, _, _ = H.truth_targets(X, periodic, 257, seed=8)
    wts, _, _ = locate(X, P, periodic)
    c = dtype(287.654321)
    got = sparse(np.full((3, X.shape[0], X.shape[1]), c, dtype=dtype), wts)
    assert np.abs(got.astype(np.float64) - np.float64(c)).max() <= 4 * np.spacing(c)


@pytest.mark.parametrize('name', ['3x4', '5x7p', 'rot24x48'])
def test_weights_reproduce_the_target(name):
    """normalise(sum w_k X_k) = P to 1e-12: 100 x the stopping step on unit-scale vectors."""
    X, periodic = H.GRIDS[name]()
    P, _, _ = H.truth_targets(X, periodic, 257, seed=9)
    _, idx, w = locate(X, P, periodic)
    nodes = H.all_nodes(X, periodic)
    p = (w[:, :, None] * np.where((idx >= 0)[:, :, None], nodes[np.maximum(idx, 0)], 0.0)).sum(axis=1)
    assert np.abs(H.normalise(p) - P).max() <= 1e-12
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=8 * EPS)


@pytest.mark.parametrize('name', ['3x4', '5x7p', 'rot24x48'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_targets_on_nodes_return_node_values(name, dtype):
    X, periodic = H.GRIDS[name]()
    wts, _, _ = locate(X, X.reshape(-1, 3), periodic)
    assert wts.n_unmapped == 0
    src = field(2, X.shape[0], X.shape[1], dtype, seed=6)
    got = sparse(src, wts)
    # (s, t) are off by at most 64 eps / (shortest chord) (test 1), so the four weights together by at most 4 x that, times
    # the values' scale; plus the rounding of the stored result
    tol = (4 * 64 * EPS / H.shortest_chord(X, periodic) + np.finfo(dtype).eps) * np.abs(src).max()
    np.testing.assert_allclose(got.astype(np.float64), src.reshape(2, -1).astype(np.float64), rtol=0, atol=tol)


def test_regular_global_grid_stays_within_the_bilinear_corners(capsys):
    """On a regular global grid handed over as 2-D coordinates every output lies within [min, max] of the four source values
    `regrid_field` uses for that target (targets at 0.25-0.75 of a cell in latitude, where the chord bulge cannot change the
    cell).  The largest difference from regrid_field is printed, nothing is asserted about it."""
    case = synthetic.make_gcm_grid_case(nlat_src=24, nlon_src=48, ntime=1, nplev=3, seed=2)
    slat, slon, src = case['src_lat'], case['src_lon'], case['field'][0]
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 23, 13)
    tlat = np.sort(slat[rows] + rng.uniform(0.25, 0.75, 13) * (slat[rows + 1] - slat[rows]))
    tlon = np.sort((rng.integers(0, 48, 20) + rng.uniform(0.1, 0.9, 20)) * 7.5)
    lat2, lon2 = np.meshgrid(slat, slon, indexing='ij')
    assert F.periodic_lon_rule(lon2)
    wts = F.curvilinear_weights(lat2, lon2, tlat, tlon, True)
    assert wts.n_unmapped == 0 and wts.targ_shape == (13, 20)
    got = F.regrid_curvilinear(src, wts)
    ref = F.regrid_field(src, slat, slon, tlat, tlon)
    tb = F.regrid_tables(slat, slon, tlat, tlon)
    corners = np.stack([src[:, tb[a]][:, :, tb[b]] for a in ('lat_lo', 'lat_hi') for b in ('lon_lo', 'lon_hi')])
    assert (got >= corners.min(axis=0)).all() and (got <= corners.max(axis=0)).all()
    with capsys.disabled():
        print('\nlargest |curvilinear - regrid_field| on a 24 x 48 regular grid: %.3e (field scale %.2f)'
              % (np.abs(got - ref).max(), np.abs(src).max()))


# ----------------------------------------------------------------------------------------------- 5. drop-in
def era_grid():
    ds = ncio.Dataset()
    lat, lon = np.linspace(34.0, 62.0, 15), np.linspace(-20.0, 50.0, 22)
    ds['lat'] = ncio.Field(lat, ('lat',), {'lat': lat}, dict(units='degrees_north'))
    ds['lon'] = ncio.Field(lon, ('lon',), {'lon': lon}, dict(units='degrees_east'))
    return ds


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_regrid_lat_lon_drop_in(dtype):
    ds = synthetic.make_rotated_delta(dtype=dtype)
    ds['hur'] = ncio.Field(ds['ta'].values * 2, ds['ta'].dims, ds['ta'].coords, dict(units='%'))
    era = era_grid()
    ctx = default_context()
    F._WEIGHTS_CACHE.clear()
    ctx.profile(True)
    try:
        ctx.profile_reset()
        out = F.regrid_lat_lon(ds, era, 'ta', i_use_xesmf=1)
        out2 = F.regrid_lat_lon(ds, era, 'hur', i_use_xesmf=1)       # same grids: no second locate
        assert ctx.profile_get('cell_locate')[0] == 1
        assert ctx.profile_get('regrid_sparse')[0] == 2
    finally:
        ctx.profile(False)
    f = out['ta']
    assert f.dims == ('time', 'plev', 'lat', 'lon') and f.shape == (2, 3, 15, 22) and f.dtype == dtype
    np.testing.assert_array_equal(out['lat'].values, era['lat'].values)
    np.testing.assert_array_equal(out['lon'].values, era['lon'].values)
    np.testing.assert_array_equal(f.coords['lat'], era['lat'].values)
    np.testing.assert_array_equal(f.coords['plev'], ds['plev'].values)
    assert out['lat'].dims == ('lat',) and out['lon'].dims == ('lon',)
    for name in ('ta', 'time', 'plev', 'lat', 'lon'):                  # attributes kept, reference functions.py:804-810
        assert out[name].attrs == ds[name].attrs, name
    assert out.attrs == ds.attrs and 'rlat' not in out and 'hur' not in out
    wts = F.curvilinear_weights(ds['lat'].values, ds['lon'].values, era['lat'].values, era['lon'].values, False)
    assert 0 < wts.n_unmapped < 15 * 22                                # the ERA5 box sticks out of the rotated domain
    same_bits(f.values, F.regrid_curvilinear(ds['ta'].values, wts))
    same_bits(out2['hur'].values, F.regrid_curvilinear(ds['hur'].values, wts))
    idx = wts.idx.numpy()
    assert (f.values.reshape(6, -1)[:, (idx == -1).all(axis=1)] == 0.0).all()
    # a 2-D target: the target's dimension names and its 2-D coordinate pair
    era2 = ncio.Dataset()
    la2, lo2 = np.meshgrid(np.linspace(45.0, 50.0, 4), np.linspace(5.0, 15.0, 6), indexing='ij')
    era2['lat'] = ncio.Field(la2 + 0.1 * lo2, ('y', 'x'))
    era2['lon'] = ncio.Field(lo2, ('y', 'x'))
    o = F.regrid_lat_lon(ds, era2, 'ta', i_use_xesmf=1)
    assert o['ta'].dims == ('time', 'plev', 'y', 'x') and o['lat'].dims == ('y', 'x') and o['lon'].shape == (4, 6)
    # i_use_xesmf = 0 still takes the separable path, which needs 1-D coordinates
    g = synthetic.make_gcm_grid_case(nlat_src=8, nlon_src=16, nlat=5, nlon=8, ntime=1, nplev=1)
    np.testing.assert_array_equal(F.regrid_field(g['field'], g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon']).shape,
                                  (1, 1, 5, 8))


def test_step02_command_line_with_the_setting_on(tmp_path):
    ds = synthetic.make_rotated_delta(dtype=np.float32)
    gcm, outd = tmp_path / 'gcm', tmp_path / 'out'
    gcm.mkdir()
    for base in settings.file_name_bases.values():
        ncio.to_netcdf(ds, str(gcm / base.format('ta')))
    era = era_grid()
    era_path = str(tmp_path / 'era5.nc')
    ncio.to_netcdf(era, era_path)
    code = ('import sys; from pgw4era5_amd import settings; settings.i_use_xesmf_regridding = 1; '
            'from pgw4era5_amd import step_02_preproc_deltas as m; m.main(sys.argv[1:])')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-c', code, 'regridding', '-i', str(gcm), '-o', str(outd), '-e', era_path, '-v', 'ta'],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'target points lie in no source cell' in r.stdout         # i_debug >= 1 prints the unmapped count
    want = F.regrid_lat_lon(ncio.open_dataset(str(gcm / 'ta_delta.nc')), ncio.open_dataset(era_path, decode_times=False), 'ta',
                            i_use_xesmf=1)
    for base in settings.file_name_bases.values():
        got = ncio.open_dataset(str(outd / base.format('ta')))
        assert got['ta'].dims == ('time', 'plev', 'lat', 'lon') and got['ta'].dtype == np.float32
        same_bits(np.asarray(got['ta'].values), np.asarray(want['ta'].values))
        np.testing.assert_array_equal(got['lat'].values, era['lat'].values)
        assert got['ta'].attrs.get('units') == 'K' and got.attrs.get('title') == ds.attrs['title']


def test_height_attributes_and_foreign_byte_order():
    """`height` (a scalar coordinate variable of near-surface fields) and its attributes are carried over (reference
    functions.py:805-808); float32 values in the file's byte order stay float32."""
    ds = synthetic.make_rotated_delta(nrlat=6, nrlon=8, nplev=1, ntime=2, dtype=np.float32, var_name='tas')
    ds['height'] = ncio.Field(np.array(2.0), (), {}, dict(units='m', positive='up'))
    native = F.regrid_lat_lon(ds, era_grid(), 'tas', i_use_xesmf=1)
    assert 'height' in native and native['height'].attrs == dict(units='m', positive='up')
    assert float(native['height'].values) == 2.0
    ds['tas'] = ncio.Field(ds['tas'].values.astype('>f4'), ds['tas'].dims, ds['tas'].coords, ds['tas'].attrs)
    swapped = F.regrid_lat_lon(ds, era_grid(), 'tas', i_use_xesmf=1)
    assert swapped['tas'].dtype == np.float32
    same_bits(np.asarray(swapped['tas'].values), np.asarray(native['tas'].values))


# ----------------------------------------------------------------------------------------------- 6. bad arguments
def test_bad_shapes_return_err_arg():
    """Bad shapes and null pointers come back as PGW_ERR_ARG (a ValueError here) before anything is launched."""
    ctx = default_context()
    X, periodic = H.GRIDS['3x4']()
    wts, _, _ = locate(X, X.reshape(-1, 3)[:5], periodic)
    src, out = ctx.to_device(np.zeros((1, 3, 4))), ctx.empty((1, 5), np.float64)
    P, Xd = ctx.to_device(X.reshape(-1, 3)[:5].copy()), ctx.to_device(X.reshape(-1, 3).copy())
    bs, bc = ctx.empty((2,), np.int32).copy_from(np.zeros(2, np.int32)), ctx.empty((1,), np.int32).copy_from(np.zeros(1, np.int32))
    n = C.c_longlong(0)

    def locate_rc(ntarg=5, ny=3, nx=4, nb=1, p=P.ptr, cnt=C.byref(n)):
        return ctx.lib.pgw_bilinear_locate(ctx.handle, ntarg, p, ny, nx, 0, Xd.ptr, nb, bs.ptr, bc.ptr, wts.idx.ptr, wts.w.ptr, cnt)

    def sparse_rc(dtype=_lib.PGW_F64, nfield=1, ny=3, nx=4, ntarg=5, s=src.ptr):
        return ctx.lib.pgw_regrid_sparse(ctx.handle, dtype, nfield, ny, nx, ntarg, s, wts.idx.ptr, wts.w.ptr, 0, out.ptr)
    assert locate_rc() == _lib.PGW_OK and sparse_rc() == _lib.PGW_OK
    for rc in (locate_rc(ntarg=0), locate_rc(ny=1), locate_rc(nx=1), locate_rc(nb=0), locate_rc(nb=513), locate_rc(p=None),
               locate_rc(cnt=None), sparse_rc(dtype=7), sparse_rc(nfield=0), sparse_rc(ny=1), sparse_rc(nx=1), sparse_rc(ntarg=0),
               sparse_rc(s=None)):
        assert rc == _lib.PGW_ERR_ARG
    with pytest.raises(ValueError):
        ctx._check(sparse_rc(ny=1))
    with pytest.raises(ValueError):
        F.locate_points(X[:1], X.reshape(-1, 3), False)
    with pytest.raises(ValueError):
        F.regrid_curvilinear(np.zeros((2, 4, 4)), wts)
    ctx.sync()
