"""Winds of a rotated-pole source grid through the curvilinear regridding on the GPU (k_row_mean_plain_wind,
k_regrid_sparse_wind; functions.regrid_curvilinear_wind, regrid_lat_lon_source_wind, `step_02 regridding --source_winds`).
The definition is the composed form through the existing entries - rotate_wind(inverse), regrid_curvilinear on each component,
rotate_wind - and every comparison is bit for bit against it, in both forms of the kernel (a block's source window staged in
LDS, or gathered directly).  source_winds_cases.statement restates the composed form in numpy."""
import os

import numpy as np
import pytest

import source_winds_cases as S
import test_regrid_curvilinear_host as H
import wind_rotation_cases as W
from pgw4era5_amd import _lib, functions as F, ncio, settings
from pgw4era5_amd import step_02_preproc_deltas as s2
from pgw4era5_amd.device import default_context

pytestmark = pytest.mark.gpu
same_bits = W.same_bits
WIN = 1024                                    # SPARSE_WIND_WIN of pgw_kernels.h
COMBOS = [(True, False), (False, True), (True, True), (False, False)]          # (source rotation, target rotation)


def fused(ua, va, wts, src=None, targ=None, direct=False, **opts):
    ctx = default_context()
    opts = dict(opts, sparse_direct=1 if direct else 0)
    old = {k: ctx.set_option(k, v) for k, v in opts.items()}
    try:
        return F.regrid_curvilinear_wind(ua, va, wts, *(src or (None, None)), *(targ or (None, None)))
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def composed(ua, va, wts, src=None, targ=None):
    u, v = F.rotate_wind(ua, va, *src, inverse=True) if src else (ua, va)
    u, v = F.regrid_curvilinear(u, wts), F.regrid_curvilinear(v, wts)
    return F.rotate_wind(u, v, *targ) if targ else (u, v)


def check_both_forms(ua, va, wts, src, targ, want=None):
    want = composed(ua, va, wts, src, targ) if want is None else want
    for direct in (False, True):
        for got, ref in zip(fused(ua, va, wts, src, targ, direct), want):
            same_bits(got, ref)
    return want


def pair(nf, ny, nx, dtype, seed):
    rng = np.random.default_rng(seed)
    return tuple((10.0 * rng.standard_normal((nf, ny, nx))).astype(dtype) for _ in range(2))


@pytest.fixture(scope='module')
def located():
    """The weights of (grid, nt), located once for the module."""
    cache = {}

    def get(name, nt):
        if (name, nt) not in cache:
            X, periodic = H.GRIDS[name]()
            cache[name, nt] = (X, F.locate_points(X, S.targets(X, periodic, nt, seed=nt), periodic))
        return cache[name, nt]
    return get


# ----------------------------------------------------------------------------------------------- 1. the composed form
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('nf', [1, 3, 17])
@pytest.mark.parametrize('nt', [1, 65, 257, 1028])
@pytest.mark.parametrize('name', ['3x4', '5x7p', 'rot24x48'])
def test_fused_equals_composed_in_both_forms(name, nt, nf, dtype, located):
    """1 / 65 / 257 targets: one value per thread, a ragged last block; 1028: vector stores, more than one block.  17 planes:
    ragged z-slices.  All four combinations of the two rotations; neither: regrid_curvilinear on each component."""
    X, wts = located(name, nt)
    ua, va = pair(nf, X.shape[0], X.shape[1], dtype, seed=nf)
    src, targ = S.angles(X.shape[:2], 5), S.angles((nt,), 6)
    for rot_s, rot_t in COMBOS:
        want = check_both_forms(ua, va, wts, src if rot_s else None, targ if rot_t else None)
        assert want[0].dtype == dtype and want[0].shape == (nf, nt)
    idx, w = wts.idx.numpy(), wts.w.numpy()
    for got, ref in zip(fused(ua, va, wts, src, targ), S.statement(ua, va, idx, w, src, targ)):   # and the numpy statement
        same_bits(got, ref)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_window_threshold(dtype):
    """The 48 x 96 source plane of test_apply_window_threshold (4608 elements) is wider than the wind kernel's window of 1024:
    scattered targets make every block gather directly on its own, targets sorted along a source row stage their window."""
    lat, lon = np.meshgrid(np.linspace(-80, 80, 48), np.arange(96) * 3.75, indexing='ij')
    X = F.unit_vectors(lat, lon)
    scattered = H.normalise(np.random.default_rng(3).standard_normal((1028, 3)))
    row = F.unit_vectors(np.full(1028, 31.3), np.linspace(1.0, 300.0, 1028))
    ua, va = pair(3, 48, 96, dtype, seed=9)
    src = S.angles((48, 96), 7)
    for P in (scattered, row):
        wts = F.locate_points(X, P, True)
        idx = wts.idx.numpy()
        check_both_forms(ua, va, wts, src, S.angles((1028,), 8))
    inner = idx[(idx >= 0).all(axis=1)]
    assert inner.max() - inner.min() < WIN                          # the row's window fits


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_nan_unmapped_and_absent_entries(dtype, monkeypatch):
    X, periodic = H.GRIDS['5x7p']()
    P = np.concatenate([S.targets(X, periodic, 120, seed=4), np.array([[np.nan, 0.0, 1.0]])], axis=0)
    wts = F.locate_points(X, P, periodic)
    idx = wts.idx.numpy()
    caps, unmapped = idx[:, 3] == -1, (idx == -1).all(axis=1)
    assert (caps & ~unmapped).any() and unmapped.any()
    ua, va = pair(3, 5, 7, dtype, seed=1)
    ua[:, 0, 0] = np.nan                       # source element 0 of ua only: beside every idx = -1 entry, which must stay unread
    ua[1, 2, 3] = np.nan
    src, targ = S.angles((5, 7), 2), S.angles((len(P),), 3)
    uses_nan = ((idx == 0) | (idx == 35)).any(axis=1)              # node 0 and the pole of row 0, whose mean holds it
    uses_mid = (idx == 2 * 7 + 3).any(axis=1)
    clean = ~uses_nan & ~uses_mid
    assert uses_nan.any() and (idx == 35).any() and uses_mid.any() and (caps & clean).any()
    for s, t in ((src, None), (src, targ), (None, targ)):
        for direct in (False, True):
            got = fused(ua, va, wts, s, t, direct)
            for g, ref in zip(got, S.statement(ua, va, idx, wts.w.numpy(), s, t)):
                same_bits(g, ref)
            if s is not None:                                      # the rotation mixes ua's NaN into both components
                for g in got:
                    assert np.isnan(g[:, uses_nan]).all() and np.isnan(g[1][uses_mid]).all()
                    assert not np.isnan(g[:, clean]).any() and not np.isnan(g[0][uses_mid & ~uses_nan]).any()
            assert (got[0][:, unmapped] == 0.0).all() and (got[1][:, unmapped] == 0.0).all()
        check_both_forms(ua, va, wts, s, t)
    monkeypatch.setattr(settings, 'xesmf_unmapped_to_nan', True)
    for direct in (False, True):
        got = fused(ua, va, wts, src, targ, direct)
        for g, ref in zip(got, S.statement(ua, va, idx, wts.w.numpy(), src, targ, unmapped_nan=True)):
            same_bits(g, ref)
            assert np.isnan(g[:, unmapped]).all()
    check_both_forms(ua, va, wts, src, targ)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_forced_single_width_gives_the_same_bits(dtype, located):
    X, wts = located('5x7p', 1028)
    ua, va = pair(3, 5, 7, dtype, seed=3)
    src, targ = S.angles((5, 7), 5), S.angles((1028,), 6)
    want = composed(ua, va, wts, src, targ)
    for direct in (False, True):
        for got, ref in zip(fused(ua, va, wts, src, targ, direct, force_vec1=1), want):
            same_bits(got, ref)


def test_solid_body_flow_comes_out_geographic():
    """The physical check of tests/test_source_winds_host.py on the GPU: grid-relative (cos rlat, 0) on the rot24x48 grid
    against regrid_curvilinear of the analytic geographic components, to 1e-13 in float64."""
    case = S.solid_body_case()
    wts = F.locate_points(case['X'], case['P'], False)
    assert wts.n_unmapped == 0
    src = F.wind_rotation(case['lat'], case['lon'], *S.SOURCE_POLE)
    got = fused(*case['grid'], wts, src)
    want = [F.regrid_curvilinear(g, wts) for g in case['geo']]
    err = max(np.abs(g - x).max() for g, x in zip(got, want))
    off = max(np.abs(g - x).max() for g, x in zip(fused(*case['grid'], wts), want))
    print('solid body on the GPU: |fused - analytic| = %.3e, without the source rotation %.3f' % (err, off))
    assert got[0].dtype == np.float64 and err <= 1e-13 and off > 0.05


# ----------------------------------------------------------------------------------------------- 2. arguments
def test_bad_arguments_return_err_arg_and_leave_the_outputs():
    ctx = default_context()
    X, periodic = H.GRIDS['3x4']()
    wts = F.locate_points(X, X.reshape(-1, 3)[:6], periodic)
    f64 = np.dtype('float64')
    su, sv = ctx.to_device(np.ones((2, 3, 4)), f64), ctx.to_device(np.ones((2, 3, 4)), f64)
    sc, ss = (ctx.to_device(x, f64) for x in S.angles((3, 4), 1))
    tc, ts = (ctx.to_device(x, f64) for x in S.angles((6,), 2))
    big = ctx.to_device(np.full(64, -7.5), f64)                     # both outputs, with room behind them
    uo, vo = big.ptr, big.ptr + 16 * 8

    def rc(dtype=_lib.PGW_F64, nfield=2, ny=3, nx=4, ntarg=6, u=su.ptr, v=sv.ptr, c=sc.ptr, s=ss.ptr, i=wts.idx.ptr, w=wts.w.ptr,
           a=tc.ptr, b=ts.ptr, uo=uo, vo=vo):
        return ctx.lib.pgw_regrid_sparse_wind(ctx.handle, dtype, nfield, ny, nx, ntarg, u, v, c, s, i, w, 0, a, b, uo, vo)
    bad = [rc(dtype=7), rc(nfield=0), rc(ny=1), rc(nx=1), rc(ntarg=0), rc(u=None), rc(v=None), rc(i=None), rc(w=None), rc(uo=None),
           rc(vo=None),
           rc(c=None), rc(s=None), rc(a=None), rc(b=None),                                 # half a pair
           rc(u=su.ptr + 4), rc(uo=uo + 4), rc(c=sc.ptr + 4), rc(b=ts.ptr + 4), rc(w=wts.w.ptr + 4), rc(i=wts.idx.ptr + 2),
           rc(uo=su.ptr), rc(vo=sv.ptr + 8), rc(uo=sc.ptr), rc(vo=ts.ptr), rc(uo=wts.w.ptr), rc(vo=wts.idx.ptr),   # output on an input
           rc(vo=uo), rc(vo=uo + 11 * 8)]                                                  # output on the other output
    assert all(r == _lib.PGW_ERR_ARG for r in bad), bad
    ctx.sync()
    np.testing.assert_array_equal(big.numpy(), -7.5)
    np.testing.assert_array_equal(su.numpy(), 1.0)
    assert rc() == _lib.PGW_OK and rc(c=None, s=None) == _lib.PGW_OK and rc(a=None, b=None, c=None, s=None) == _lib.PGW_OK
    ctx.sync()
    out = big.numpy()
    assert (out[:12] != -7.5).all() and (out[16:28] != -7.5).all() and (out[12:16] == -7.5).all() and (out[28:] == -7.5).all()
    with pytest.raises(ValueError):
        ctx._check(rc(c=None))


def test_shape_dtype_and_array_kind_rules(located):
    ctx = default_context()
    X, wts = located('3x4', 65)
    ua, va = pair(2, 3, 4, np.float32, seed=1)
    src, targ = S.angles((3, 4), 1), S.angles((65,), 2)
    for bad in (lambda: F.regrid_curvilinear_wind(ua, va[:1], wts), lambda: F.regrid_curvilinear_wind(ua[:, :2], va[:, :2], wts),
                lambda: F.regrid_curvilinear_wind(ua[0, 0], va[0, 0], wts), lambda: F.regrid_curvilinear_wind(ua[:0], va[:0], wts),
                lambda: F.regrid_curvilinear_wind(ua, va, wts, src_cos=src[0]),
                lambda: F.regrid_curvilinear_wind(ua, va, wts, targ_sin=targ[1]),
                lambda: F.regrid_curvilinear_wind(ua, va, wts, src[0][:2], src[1][:2]),
                lambda: F.regrid_curvilinear_wind(ua, va, wts, src[0], src[1].T),
                lambda: F.regrid_curvilinear_wind(ua, va, wts, None, None, targ[0][:64], targ[1][:64]),
                lambda: F.regrid_curvilinear_wind(ua, va, wts, targ[0], targ[1], src[0], src[1])):
        with pytest.raises(ValueError):
            bad()
    u, v = F.regrid_curvilinear_wind(ua, va, wts, *src, *targ)
    assert type(u) is np.ndarray and u.dtype == v.dtype == np.float32 and u.shape == v.shape == (2, 65)
    u4, v4 = F.regrid_curvilinear_wind(ua.reshape(2, 1, 3, 4), va.reshape(2, 1, 3, 4), wts, *src, *targ)
    assert u4.shape == (2, 1, 65)
    same_bits(u4[:, 0], u)
    um, vm = F.regrid_curvilinear_wind(ua, va.astype(np.float64), wts, *src, *targ)      # float32 only when both are
    assert um.dtype == vm.dtype == np.float64
    for got, ref in zip((um, vm), composed(ua, va.astype(np.float64), wts, src, targ)):
        same_bits(got, ref)
    du, dv = ctx.to_device(ua, np.dtype('float32')), ctx.to_device(va, np.dtype('float32'))
    dc, ds = (ctx.to_device(x, np.dtype('float64')) for x in src)
    gu, gv = F.regrid_curvilinear_wind(du, dv, wts, dc, ds, *targ)
    assert type(gu).__name__ == 'DeviceArray' and gu.shape == (2, 65)
    same_bits(gu.numpy(), u)
    same_bits(gv.numpy(), v)
    with pytest.raises(TypeError):
        F.regrid_curvilinear_wind(du, ctx.to_device(va.astype(np.float64), np.dtype('float64')), wts)
    # a labelled ua keeps its labels (the same 65 targets as a 5 x 13 target grid: as many dimensions out as in)
    wts2 = F.CurvilinearWeights(wts.idx, wts.w, wts.n_unmapped, wts.src_shape, (5, 13), wts.periodic)
    lu = ncio.Field(ua, ('time', 'y', 'x'), {'time': np.arange(2)})
    fu, fv = F.regrid_curvilinear_wind(lu, va, wts2, *src, *(t.reshape(5, 13) for t in targ))
    assert type(fv) is np.ndarray and fv.shape == (2, 5, 13) and fu.dims == ('time', 'y', 'x')
    same_bits(np.asarray(fu.values).reshape(2, 65), u)


# ----------------------------------------------------------------------------------------------- 3. step_02
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('source_winds_hip'))
    return dict(tmp=tmp, gcm=S.write_sources(os.path.join(tmp, 'gcm')), mesh=S.write_mesh_target(os.path.join(tmp, 'mesh.nc')),
                rotated=S.write_rotated_target(os.path.join(tmp, 'rotated.nc')))


def run(files, name, target, *flags, variables='ua,va,ta'):
    out = os.path.join(files['tmp'], 'out_' + name)
    done = s2.main(['regridding', '-i', files['gcm'], '-o', out, '-e', target, '-v', variables] + list(flags))
    assert sorted(os.path.basename(p) for p in done) == sorted(b.format(v) for b in settings.file_name_bases.values()
                                                               for v in variables.split(','))
    return out


def opened(directory, base, var):
    return ncio.open_dataset(os.path.join(directory, base.format(var)))


def wind_inputs(files, base):
    ds_u, ds_v = opened(files['gcm'], base, 'ua'), opened(files['gcm'], base, 'va')
    return ds_u, ds_v, np.ascontiguousarray(ds_u['ua'].values), np.ascontiguousarray(ds_v['va'].values)


def test_step02_source_winds_onto_a_mesh(files, monkeypatch):
    monkeypatch.setattr(settings, 'i_use_xesmf_regridding', 1)
    out, plain = run(files, 'mesh_auto', files['mesh'], '--source_winds'), run(files, 'mesh_plain', files['mesh'])
    era = ncio.open_dataset(files['mesh'], decode_times=False)
    for base in settings.file_name_bases.values():
        ds_u, ds_v, ua, va = wind_inputs(files, base)
        want = F.regrid_lat_lon_source_wind(ds_u, ds_v, era, S.SOURCE_POLE, None)
        wts = F.curvilinear_weights(ds_u['lat'].values, ds_u['lon'].values, era['lat'].values, era['lon'].values, False)
        assert wts.n_unmapped == 0
        src = F.wind_rotation(np.asarray(ds_u['lat'].values, dtype=np.float64), np.asarray(ds_u['lon'].values, dtype=np.float64),
                              *S.SOURCE_POLE)
        comp = composed(ua, va, wts, src)
        for k, var in enumerate(('ua', 'va')):
            got, ref = opened(out, base, var), opened(plain, base, var)
            assert got[var].dtype == np.float32 and got[var].dims == ('time', 'plev', 'lat', 'lon')
            same_bits(np.asarray(got[var].values), np.asarray(want[k][var].values))
            same_bits(np.asarray(got[var].values), comp[k])
            assert 'wind_components' not in got[var].attrs and 'grid_north_pole_latitude' not in got[var].attrs
            assert got[var].attrs == ref[var].attrs and got.attrs == ref.attrs and sorted(got.variables) == sorted(ref.variables)
            assert np.abs(np.asarray(got[var].values) - np.asarray(ref[var].values)).max() > 0.01      # the rotation did act
        with open(os.path.join(out, base.format('ta')), 'rb') as a, open(os.path.join(plain, base.format('ta')), 'rb') as b:
            assert a.read() == b.read()


def test_step02_source_winds_onto_a_rotated_target(files, monkeypatch):
    monkeypatch.setattr(settings, 'i_use_xesmf_regridding', 1)
    out = run(files, 'rotated', files['rotated'], '--source_winds', '39.25,-162', '--rotate_winds', variables='ua,va')
    era = ncio.open_dataset(files['rotated'], decode_times=False)
    tlat, tlon = (np.asarray(era[c].values, dtype=np.float64) for c in ('lat', 'lon'))
    for base in settings.file_name_bases.values():
        ds_u, ds_v, ua, va = wind_inputs(files, base)
        wts = F.curvilinear_weights(ds_u['lat'].values, ds_u['lon'].values, tlat, tlon, False)
        src = F.wind_rotation(np.asarray(ds_u['lat'].values, dtype=np.float64), np.asarray(ds_u['lon'].values, dtype=np.float64),
                              *S.SOURCE_POLE)
        comp = composed(ua, va, wts, src, F.wind_rotation(tlat, tlon, *S.TARGET_POLE))
        for k, var in enumerate(('ua', 'va')):
            got = opened(out, base, var)
            assert got[var].dims == ('time', 'plev', 'rlat', 'rlon') and got['lat'].dims == ('rlat', 'rlon')
            same_bits(np.asarray(got[var].values), comp[k])
            assert got[var].attrs['wind_components'] == 'grid_relative' and got[var].attrs['units'] == 'K'
            assert (float(got[var].attrs['grid_north_pole_latitude']), float(got[var].attrs['grid_north_pole_longitude'])) == S.TARGET_POLE
    # a source variable that carries the marker already is accepted: the flag states what the marker states
    base = settings.file_name_bases['SCEN-HIST']
    again = F.regrid_lat_lon_source_wind(opened(out, base, 'ua'), opened(out, base, 'va'),
                                         ncio.open_dataset(files['mesh'], decode_times=False), S.TARGET_POLE, None)
    assert 'wind_components' not in again[0]['ua'].attrs and 'grid_north_pole_latitude' not in again[1]['va'].attrs


def test_step02_without_the_flags_is_unchanged(files, monkeypatch):
    monkeypatch.setattr(settings, 'i_use_xesmf_regridding', 1)
    out = run(files, 'plain', files['mesh'])
    era = ncio.open_dataset(files['mesh'], decode_times=False)
    for base in settings.file_name_bases.values():
        for var in ('ua', 'va', 'ta'):
            want = F.interp_wrapper(opened(files['gcm'], base, var), era, var, i_use_xesmf=1,
                                    nan_interp_kernel_radius=settings.nan_interp_kernel_radius,
                                    nan_interp_sharpness=settings.nan_interp_sharpness)
            ref = os.path.join(files['tmp'], 'ref_' + base.format(var))
            ncio.to_netcdf(want, ref)
            with open(os.path.join(out, base.format(var)), 'rb') as a, open(ref, 'rb') as b:
                assert a.read() == b.read()
