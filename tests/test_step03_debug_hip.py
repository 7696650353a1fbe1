"""GPU tests of step_03 --debug_mode: `pgw_delta_fields` (k_delta_fields), `pgw_surface_deltas` and the two file functions.

The deltas the debug mode writes are the ones production adds: the kernel is checked against the oracles on odd shapes,
against production bit for bit (era + delta in numpy == the outputs of the per-file path), against the composed
function-level entries bit for bit, and for its errors; then the command line on float32 files."""
import datetime as dt
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from surface_edge_cases import oracle_surface_deltas                                 # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = {'1x1': (1, 1),          # one column: one live lane
         '6x11': (6, 11),        # 66 columns: one wave + 2 lanes
         '8x12': (8, 12)}        # 96 columns: one and a half waves
INSTANTS = {'lerp': None,                                  # make_case's default instant: between two records
            'record': dt.datetime(2006, 3, 15, 12)}        # exactly a record: the LERP = false instantiations
PLEVS = {19: None,                                         # synthetic.PLEV19
         5: [100000., 85000., 50000., 30000., 10000.],
         2: [100000., 30000.]}
MODES = ('f64', 'f32_reference', 'f32_fast')
DTYPE = dict(f64=np.float64, f32_fast=np.float32, f32_reference=np.float32)
VARS = ('ta', 'hur', 'ua', 'va')


@pytest.fixture(scope='module')
def gpu():
    from pgw4era5_amd import step_03_apply_to_era as s3, step_03_debug as dbg
    from pgw4era5_amd.device import default_context
    return s3, dbg, default_context()


@functools.lru_cache(maxsize=None)
def make(grid, nlev, nplev, dtype_name, instant, seed=31):
    from pgw4era5_amd import synthetic
    nlat, nlon = GRIDS[grid]
    kw = {} if INSTANTS[instant] is None else dict(target_dt=INSTANTS[instant])
    return synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=seed, dtype=np.dtype(dtype_name).type, plev=PLEVS[nplev], **kw)


def tie_deltas(c):
    """The deltas with ps_hist ON pressure levels, one ulp beside them and above all of them (the ties of the surface rule,
    functions.py:356-365), in columns next to each other, on both sides of the wave boundary and at the end of the grid."""
    dtype = c['deltas']['ps_hist'].dtype.type
    p = np.sort(np.asarray(c['plev'])).astype(dtype)
    d = {k: v.copy() for k, v in c['deltas'].items()}
    flat = d['ps_hist'].reshape(12, -1)
    ncol = flat.shape[1]
    values = [p[-1], p[-2], np.nextafter(p[-1], dtype(np.inf)), p[-3], np.nextafter(p[-2], dtype(0)), p[-4], dtype(103000.0),
              p[-6], np.nextafter(p[0], dtype(np.inf)), p[1]]
    for col, v in zip([0, 1, 7, 18, 29, 40, 51, 63, 64, ncol - 1], values):
        flat[:, col] = v
    return d


def widen(x):
    return {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in x.items()}


def device_fields(gpu, c, deltas, mode, ps=None, ignore_top=True, opts=None):
    """pgw_delta_fields on the records of `deltas` and the levels of `ps` (default: the file's PS) -> dict of numpy float64."""
    s3, dbg, ctx = gpu
    dtype = np.dtype(DTYPE[mode])
    era = c['era']
    ctx.set_levels(era['ak'], era['bk'], era.get('akm'), era.get('bkm'))
    ds = s3.DeltaSet(ctx, deltas, c['delta_times'], c['plev'], dtype)
    ps_dev = ctx.to_device(np.ascontiguousarray(era['PS'] if ps is None else ps, dtype=dtype), dtype)
    old = {k: ctx.set_option(k, v) for k, v in (opts or {}).items()}
    try:
        out = dbg.delta_fields_device(ctx, ps_dev, ds, c['target_dt'], era['T'].shape[1], mode == 'f32_reference', ignore_top)
        return {k: v.numpy() for k, v in out.items()}
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
        ds.free()


def oracle_fields(c, deltas, mode, ps=None):
    """load_delta_interp of the four variables by the oracle of the mode (fast float32: the float64 oracle on the stored values)."""
    era = c['era']
    ps = era['PS'] if ps is None else ps
    if mode == 'f32_reference':
        _, pa = R.hybrid_pressure(era['ak'], era['bk'], ps)
        ld = lambda k: R.load_delta_values(deltas[k], c['delta_times'], c['target_dt'])
        vi = R.vert_interp_delta
    else:
        _, pa = O.hybrid_pressure(era['ak'], era['bk'], np.asarray(ps, dtype=np.float64))
        ld = lambda k: O.load_delta_values(np.asarray(deltas[k], dtype=np.float64), c['delta_times'], c['target_dt'])
        vi = O.vert_interp_delta
    out = {}
    for var in VARS:
        sfc, psh = (ld(var + 's'), ld('ps_hist')) if var in ('ta', 'hur') else (None, None)
        out[var] = vi(ld(var), c['plev'], pa, sfc, psh, True)
    return out


# ================================================================== 1. the kernel against the oracles
@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_delta_fields_vs_oracle(gpu, mode, grid, instant):
    """float64 records against O.vert_interp_delta, float32 records (ref_dtype = 1) against R.vert_interp_delta, fed
    load_delta_values of the same records: rtol = atol = 1e-9 (float64 fields against these oracles, tests/test_hip_files.py).
    1, 66 and 96 columns; 1, 12 and 21 levels; 2, 5 and 19 pressure levels; 32- and 64-bit byte offsets."""
    for nlev in (1, 12, 21):
        for nplev in (2, 5, 19):
            c = make(grid, nlev, nplev, np.dtype(DTYPE[mode]).name, instant)
            want = oracle_fields(c, c['deltas'], mode)
            for off64 in (0, 1):
                got = device_fields(gpu, c, c['deltas'], mode, opts=dict(force_off64=off64))
                for var in VARS:
                    assert got[var].dtype == np.float64 and got[var].shape == want[var].shape
                    np.testing.assert_allclose(got[var], want[var], rtol=1e-9, atol=1e-9,
                                               err_msg='%s nlev %d nplev %d off64 %d' % (var, nlev, nplev, off64))


# ================================================================== 2. bit for bit what production adds
@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', ['6x11', '8x12'])
@pytest.mark.parametrize('mode', MODES)
def test_era_plus_delta_is_production_bit_for_bit(gpu, mode, grid, instant):
    """era + delta in numpy float64 (float32 files: float64(field) + delta; fast mode: that sum cast to float32) equals the T, U, V
    the per-file path returns, on the tie columns of the surface rule too - with 32- and 64-bit byte offsets on both sides and,
    for float64 files, with and without the loop's first scans in the production kernel (fused_first), so every production
    instantiation of the delta walk is held to the fields kernel's.  dhur has no ERA-state output to be added to (RELHUM of
    the ERA state is not an output): it is compared with the oracle, at test 1's tolerance."""
    s3, dbg, ctx = gpu
    c = make(grid, 21, 19, np.dtype(DTYPE[mode]).name, instant)
    deltas = tie_deltas(c)
    want = oracle_fields(c, deltas, mode)
    for off64 in (0, 1):
        got = device_fields(gpu, c, deltas, mode, opts=dict(force_off64=off64))
        for fused in ((0, 1) if mode == 'f64' else (None,)):
            opts = dict(force_off64=off64) if fused is None else dict(force_off64=off64, fused_first=fused)
            old = {k: ctx.set_option(k, v) for k, v in opts.items()}
            try:
                prod = s3.pgw_for_era5_arrays(c['era'], deltas, c['delta_times'], c['plev'], c['target_dt'], True,
                                              ref_dtype=dict(f64=None, f32_fast=False, f32_reference=True)[mode])
            finally:
                for k, v in old.items():
                    ctx.set_option(k, v)
            for var, name in (('ta', 'T'), ('ua', 'U'), ('va', 'V')):
                total = np.asarray(c['era'][name], dtype=np.float64) + got[var]
                if mode == 'f32_fast':
                    total = total.astype(np.float32)
                assert prod[name].dtype == total.dtype
                np.testing.assert_array_equal(total, prod[name], err_msg='%s off64 %d fused_first %s' % (name, off64, fused))
        np.testing.assert_allclose(got['hur'], want['hur'], rtol=1e-9, atol=1e-9, err_msg='hur off64 %d' % off64)


# ================================================================== 3. bit for bit the composed entries
def composed_common_f64(gpu, c, deltas):
    """Four pgw_vert_interp_delta calls (records and abscissae in, add_to = NULL) on the levels of the file's PS."""
    s3, dbg, ctx = gpu
    from pgw4era5_amd import _lib
    era = c['era']
    f64 = np.dtype('float64')
    ctx.set_levels(era['ak'], era['bk'])
    ds = s3.DeltaSet(ctx, deltas, c['delta_times'], c['plev'], f64)
    ps = ctx.to_device(np.ascontiguousarray(era['PS'], dtype=f64), f64)
    nt, N, nlat, nlon = era['T'].shape
    plev = ds.plev
    out = {}
    try:
        for var in VARS:
            b, a, x_hi, x_new = ds.pair(var, c['target_dt'], None)
            sfc = [None] * 4
            if var in ('ta', 'hur'):
                sb, sa, _, _ = ds.pair(var + 's', c['target_dt'], None)
                pb, pa, _, _ = ds.pair('ps_hist', c['target_dt'], None)
                sfc = [sb.ptr, sa.ptr, pb.ptr, pa.ptr]
            o = ctx.empty((nt, N, nlat, nlon), f64)
            ctx._check(ctx.lib.pgw_vert_interp_delta(ctx.handle, _lib.PGW_F64, nt, len(plev), N, nlat * nlon, plev.ctypes.data_as(_lib._dp),
                                                     b.ptr, a.ptr, x_hi, x_new, *sfc, None, ps.ptr, 1, None, o.ptr))
            out[var] = o.numpy()
    finally:
        ds.free()
    return out


def composed_reference_f32(gpu, c, deltas):
    """pgw_vert_interp_delta_mixed fed pgw_time_lerp_mixed results (an exact record: the float32 record itself) on the float64
    pressures akm + float64(PS) * bkm."""
    s3, dbg, ctx = gpu
    from pgw4era5_amd import _lib
    era = c['era']
    f32, f64 = np.dtype('float32'), np.dtype('float64')
    ctx.set_levels(era['ak'], era['bk'])
    nt, N, nlat, nlon = era['T'].shape
    akm, bkm = np.empty(N), np.empty(N)
    ctx._check(ctx.lib.pgw_get_full_level_coeffs(ctx.handle, akm.ctypes.data_as(_lib._dp), bkm.ctypes.data_as(_lib._dp)))
    pa = ctx.to_device(akm[None, :, None, None] + np.asarray(era['PS'], dtype=np.float64)[:, None] * bkm[None, :, None, None], f64)
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(c['delta_times'], c['target_dt'])
    plev = np.ascontiguousarray(c['plev'], dtype=np.float64)

    def at_instant(name):
        b = ctx.to_device(np.ascontiguousarray(deltas[name][keep[ib]], dtype=f32), f32)
        if x_hi == 0.0:
            return b, _lib.PGW_F32
        a = ctx.to_device(np.ascontiguousarray(deltas[name][keep[ia]], dtype=f32), f32)
        o = ctx.empty(b.shape, f64)
        ctx._check(ctx.lib.pgw_time_lerp_mixed(ctx.handle, _lib.PGW_F32, _lib.PGW_F32, b.size, b.ptr, a.ptr, x_hi, x_new, o.ptr))
        return o, _lib.PGW_F64

    out = {}
    for var in VARS:
        d, td = at_instant(var)
        s_ptr = p_ptr = None
        ts = tp = _lib.PGW_F64
        if var in ('ta', 'hur'):
            s, ts = at_instant(var + 's')
            p, tp = at_instant('ps_hist')
            s_ptr, p_ptr = s.ptr, p.ptr
        o = ctx.empty((nt, N, nlat, nlon), f64)
        ctx._check(ctx.lib.pgw_vert_interp_delta_mixed(ctx.handle, td, ts, tp, _lib.PGW_F64, _lib.PGW_F64, nt, len(plev), N, nlat * nlon,
                                                       plev.ctypes.data_as(_lib._dp), d.ptr, s_ptr, p_ptr, pa.ptr, 1, None, o.ptr))
        out[var] = o.numpy()
    return out


@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', ['6x11', '8x12'])
@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_delta_fields_equal_the_composed_entries(gpu, mode, grid, instant):
    """One launch against the function-level composition the library already had, on the tie list of the surface rule
    (ps_hist on a level, one ulp beside it, above all levels): equal bits, 32- and 64-bit offsets."""
    c = make(grid, 21, 19, np.dtype(DTYPE[mode]).name, instant)
    deltas = tie_deltas(c)
    want = composed_common_f64(gpu, c, deltas) if mode == 'f64' else composed_reference_f32(gpu, c, deltas)
    for off64 in (0, 1):
        got = device_fields(gpu, c, deltas, mode, opts=dict(force_off64=off64))
        for var in VARS:
            np.testing.assert_array_equal(got[var], want[var], err_msg='%s off64 %d' % (var, off64))


# ================================================================== 4. errors
def _raises(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value), getattr(e.value, 'column', None), getattr(e.value, 'status', None)


@pytest.mark.parametrize('what', ['ps_hist == min(plev)', 'NaN ps_hist', 'model top above the delta top'])
def test_errors_are_those_of_vert_interp_delta(gpu, what):
    """Same exception, same message, same pgw_error_column as pgw_vert_interp_delta (ta with its surface insertion) on the
    same inputs."""
    s3, dbg, ctx = gpu
    from pgw4era5_amd import _lib
    c = make('6x11', 21, 19, 'float64', 'lerp')
    deltas = {k: v.copy() for k, v in c['deltas'].items()}
    col, ignore_top = 64, True
    if what == 'ps_hist == min(plev)':
        deltas['ps_hist'].reshape(12, -1)[:, col] = np.min(c['plev'])
    elif what == 'NaN ps_hist':
        deltas['ps_hist'].reshape(12, -1)[:, col] = np.nan
    else:
        col, ignore_top = -1, False

    def composed():
        era = c['era']
        f64 = np.dtype('float64')
        ctx.set_levels(era['ak'], era['bk'])
        ds = s3.DeltaSet(ctx, deltas, c['delta_times'], c['plev'], f64)
        ps = ctx.to_device(np.ascontiguousarray(era['PS'], dtype=f64), f64)
        nt, N, nlat, nlon = era['T'].shape
        try:
            b, a, x_hi, x_new = ds.pair('ta', c['target_dt'], None)
            sb, sa, _, _ = ds.pair('tas', c['target_dt'], None)
            pb, pa, _, _ = ds.pair('ps_hist', c['target_dt'], None)
            o = ctx.empty((nt, N, nlat, nlon), f64)
            ctx._check(ctx.lib.pgw_vert_interp_delta(ctx.handle, _lib.PGW_F64, nt, len(ds.plev), N, nlat * nlon,
                                                     ds.plev.ctypes.data_as(_lib._dp), b.ptr, a.ptr, x_hi, x_new, sb.ptr, sa.ptr,
                                                     pb.ptr, pa.ptr, None, ps.ptr, 1 if ignore_top else 0, None, o.ptr))
        finally:
            ds.free()

    want = _raises(composed)
    got = _raises(lambda: device_fields(gpu, c, deltas, 'f64', ignore_top=ignore_top))
    assert got == want, what
    assert got[1] == col
    if what == 'model top above the delta top':
        assert 'ERA5 top pressure is lower than climate delta top pressure' in got[0]
    else:
        assert got[0] == ''                                   # the reference's bare ValueError (functions.py:360-361)


# ================================================================== 5. surface deltas
# oracle_surface_deltas (step_03:103-125, 139-143 by the oracle lines of the mode) lives in tests/surface_edge_cases.py, shared
# with tests/test_surface_riders_hip.py


@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', ['6x11', '8x12'])
@pytest.mark.parametrize('mode', MODES)
def test_surface_deltas_vs_oracle(gpu, mode, grid, instant):
    """delta_ts_combined and delta_soilt as float64 arrays against integrate_tos / sea_ice_update / soil_temperature_delta
    (R.integrate_tos and the in-place float32 sea-ice update on float32 files in reference mode), NaN tos over land:
    rtol = atol = 1e-9 in every mode - the float32 nodes of reference mode (the exact-record blend included) are float32
    operations on both sides."""
    s3, dbg, ctx = gpu
    dtype = np.dtype(DTYPE[mode])
    c = make(grid, 12, 19, dtype.name, instant)
    assert np.isnan(c['deltas']['tos']).any() and not np.isnan(c['deltas']['tos']).all()
    ds = s3.DeltaSet(ctx, c['deltas'], c['delta_times'], c['plev'], dtype)
    clim = ds.ts_clim.numpy()
    era = {k: ctx.to_device(np.ascontiguousarray(c['era'][k], dtype=dtype), dtype) for k in ('FR_SEA_ICE', 'FR_LAND')}
    try:
        ts, st = dbg.surface_deltas_device(ctx, era, dict(soil1=c['era']['soil1']), ds, c['target_dt'], mode == 'f32_reference')
        ts, st = ts.numpy(), st.numpy()
    finally:
        ds.free()
    want_ts, want_st = oracle_surface_deltas(c, mode, clim if mode == 'f32_reference' else clim.astype(np.float64))
    assert ts.dtype == np.float64 and st.dtype == np.float64 and st.shape == want_st.shape
    assert np.isfinite(ts).all()
    print('%s %s %s: max rel dts %.3e, dsoil %.3e' % (mode, grid, instant, np.max(np.abs(ts - want_ts) / np.abs(want_ts)),
                                                      np.max(np.abs(st - want_st) / np.abs(want_st))))
    np.testing.assert_allclose(ts, want_ts, rtol=1e-9, atol=1e-9, err_msg='delta_ts_combined')
    np.testing.assert_allclose(st, want_st, rtol=1e-9, atol=1e-9, err_msg='delta_soilt')


# ================================================================== 6. the command line
STEPS = (dt.datetime(2006, 8, 2, 0), dt.datetime(2006, 8, 2, 3))
RECORD_STEP = dt.datetime(2006, 8, 15, 12)                    # a record of the monthly deltas: the exact-hit time step


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """Two float32 files 6 x 8 x 12 (as tests/test_hip_files.py builds them), a third at a delta record's stamp, and a
    ps_delta.nc next to the other delta files."""
    from pgw4era5_amd import synthetic, ncio
    root = tmp_path_factory.mktemp('pgw_debug')
    cases = []
    for t in STEPS + (RECORD_STEP,):
        c = synthetic.make_case(6, 8, 12, seed=11, dtype=np.float32, target_dt=t)
        synthetic.write_case_files(c, str(root / 'era'), str(root / 'deltas'))
        cases.append(c)
    c = cases[0]
    ps_delta = (c['deltas']['ps_hist'] * np.float32(0.002) * np.arange(1, 13, dtype=np.float32)[:, None, None]).astype(np.float32)
    src = ncio.open_dataset(str(root / 'deltas' / 'ps_historical.nc'), decode_times=False)
    ds = ncio.Dataset()
    for k in ('time', 'lat', 'lon'):
        ds[k] = ncio.Field(src[k].values, (k,), {}, src[k].attrs)
    ds['ps'] = ncio.Field(ps_delta, ('time', 'lat', 'lon'), attrs=dict(units='Pa'))
    ncio.to_netcdf(ds, str(root / 'deltas' / 'ps_delta.nc'))
    return root, cases, ps_delta


FULL_NAMES = ('PS', 'T', 'RELHUM', 'U', 'V', 'T_SO', 'T_SKIN')


def _read_full(out_dir, c):
    from pgw4era5_amd import ncio
    stamp = 'cas{:%Y%m%d%H}0000.nc'.format(c['target_dt'])
    return {n: ncio.open_dataset(os.path.join(out_dir, '%s_delta_%s' % (n, stamp)), decode_times=False) for n in FULL_NAMES}


def _r_deltas(c, ps):
    ld = lambda k: R.load_delta_values(c['deltas'][k], c['delta_times'], c['target_dt'])
    _, pa = R.hybrid_pressure(c['era']['ak'], c['era']['bk'], ps)
    out = {}
    for var in VARS:
        sfc, psh = (ld(var + 's'), ld('ps_hist')) if var in ('ta', 'hur') else (None, None)
        out[var] = R.vert_interp_delta(ld(var), c['plev'], pa, sfc, psh, True)
    return out


def _check_full_files(got, c, want, level_deltas, tol4):
    """Names, dtypes, dims, coordinates; contents against the oracle.  tol4: var -> (rtol, atol) of the four level deltas."""
    era = c['era']
    assert got['PS']['PS'].values.dtype == np.float32                     # ps_pgw - PS in the file's dtype (step_03:326)
    for n in FULL_NAMES[1:]:
        assert got[n][n].values.dtype == np.float64, n
    assert got['T']['T'].dims == ('time', 'level', 'lat', 'lon') and got['T_SO']['T_SO'].dims == ('time', 'soil1', 'lat', 'lon')
    assert got['PS']['PS'].dims == got['T_SKIN']['T_SKIN'].dims == ('time', 'lat', 'lon')
    np.testing.assert_array_equal(got['T']['lat'].values, c['lat'])
    np.testing.assert_array_equal(got['T_SO']['soil1'].values, era['soil1'])
    assert 'seconds since' in got['U']['time'].attrs['units'] and got['T']['T'].attrs['grid_mapping'] == 'rotated_pole'
    for var, n in zip(VARS, ('T', 'RELHUM', 'U', 'V')):
        np.testing.assert_allclose(got[n][n].values, level_deltas[var], rtol=tol4[var][0], atol=tol4[var][1], err_msg=n)
    # PS agrees with the oracle to one float32 ulp (rtol 1.3e-7, tests/test_hip_files.py::test_step03_cli_end_to_end), so the
    # difference of two surface pressures agrees to that much of the pressure itself
    np.testing.assert_allclose(got['PS']['PS'].values, want['PS'] - era['PS'], rtol=0, atol=1.3e-7 * float(np.max(want['PS'])),
                               err_msg='PS_delta')
    # the riders: the skin / soil temperature the oracle writes minus the file's, i.e. its deltas, at the rider tolerance of
    # the fields (1.3e-7 relative, one float32 ulp) taken over the deltas themselves: the annual-mean ts delta is the
    # float64 mean rounded to float32 here and numpy's float32 mean in the oracle
    ld = lambda k: R.load_delta_values(c['deltas'][k], c['delta_times'], c['target_dt'])
    comb = R.integrate_tos(ld('tos'), ld('ts'), np.asarray(era['FR_LAND'])[0], want['FR_SEA_ICE'][0])
    clim = R.load_delta_values(c['deltas']['ts'], c['delta_times'], None).mean(axis=0)
    np.testing.assert_allclose(got['T_SKIN']['T_SKIN'].values, comb, rtol=1e-9, atol=1e-9, err_msg='T_SKIN_delta')
    np.testing.assert_allclose(got['T_SO']['T_SO'].values, O.soil_temperature_delta(comb, clim, era['soil1']), rtol=1.3e-7, atol=0,
                               err_msg='T_SO_delta')


def test_cli_interpolate_full(gpu, files):
    """-D interpolate_full on two float32 files at -p 1: exactly the seven files per time step and no ERA5 file; PS_delta in
    the file's float32, the rest float64; contents as in tests 1, 2 and 5; the oracle's pass counts."""
    s3, dbg, ctx = gpu
    root, cases, _ = files
    out_dir = str(root / 'out_full')
    n_iters = s3._cli(['-i', str(root / 'era'), '-o', out_dir, '-d', str(root / 'deltas'), '-f', '2006080200', '-l', '2006080203',
                       '-H', '3', '-p', '1', '-t', '-D', 'interpolate_full'])
    stamps = ['cas{:%Y%m%d%H}0000.nc'.format(t) for t in STEPS]
    assert sorted(os.listdir(out_dir)) == sorted('%s_delta_%s' % (n, s) for n in FULL_NAMES for s in stamps)
    assert len(n_iters) == 2
    tol4 = {v: (1e-9, 1e-9) for v in VARS}
    for c, n in zip(cases[:2], n_iters):
        want = R.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
        assert n == want['n_iter']
        got = _read_full(out_dir, c)
        _check_full_files(got, c, want, _r_deltas(c, c['era']['PS']), tol4)
        prod = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
        for n4 in ('T', 'U', 'V'):                                        # float64(float32 field) + delta == production
            np.testing.assert_array_equal(np.asarray(c['era'][n4], dtype=np.float64) + got[n4][n4].values, prod[n4], err_msg=n4)
        np.testing.assert_array_equal(got['PS']['PS'].values, prod['PS'] - c['era']['PS'])
    # the direct call does the same for one file
    c = cases[0]
    direct = str(root / 'out_direct')
    os.makedirs(direct)
    n = s3.pgw_for_era5(os.path.join(str(root / 'era'), stamps[0]), os.path.join(direct, stamps[0]), str(root / 'deltas'),
                        c['target_dt'], True, debug_mode='interpolate_full')
    assert n == n_iters[0]
    assert sorted(os.listdir(direct)) == sorted('%s_delta_%s' % (k, stamps[0]) for k in FULL_NAMES)
    a, b = _read_full(direct, c), _read_full(out_dir, c)
    for k in FULL_NAMES:
        np.testing.assert_array_equal(a[k][k].values, b[k][k].values, err_msg=k)


def test_cli_interpolate_full_with_i_reinterp(gpu, files, monkeypatch):
    """settings.i_reinterp = 1: the level deltas stand on the converged surface pressure (step_03:212-216, 336-343), checked
    against R.vert_interp_delta on the oracle's final PS.  That PS agrees with ours to 2.5e-7 only, so the level deltas take
    the bounds tests/test_hip_files.py::test_step03_cli_with_i_reinterp_on_float32_files gives the fields they are part of,
    as absolute figures: T rtol 6e-8 of T (the coldest level sets it), U and V atol 2e-5; RELHUM has no assert there - its
    delta is interpolated like the wind deltas from values of the same size (|delta| <= 5) over the same pressure shift
    and takes their 2e-5 (the oracle's own deltas on these files move by 1.3e-6 (ta) and 2.6e-6 (hur) when its final PS
    moves by 2.5e-7 of its value, either way)."""
    from pgw4era5_amd import settings as S
    s3, dbg, ctx = gpu
    root, cases, _ = files
    monkeypatch.setattr(S, 'i_reinterp', 1)
    out_dir = str(root / 'out_full_reinterp')
    n_iters = s3._cli(['-i', str(root / 'era'), '-o', out_dir, '-d', str(root / 'deltas'), '-f', '2006080200', '-l', '2006080203',
                       '-H', '3', '-p', '1', '-t', '-D', 'interpolate_full'])
    assert len(os.listdir(out_dir)) == 14 and not [f for f in os.listdir(out_dir) if f.startswith('cas')]
    for c, n in zip(cases[:2], n_iters):
        want = R.pgw_for_era5_arrays_reinterp(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref=30000.0)
        assert n == want['n_iter']
        t_atol = 6e-8 * float(np.min(np.abs(want['T'])))
        tol4 = dict(ta=(0, t_atol), hur=(0, 2e-5), ua=(0, 2e-5), va=(0, 2e-5))
        got = _read_full(out_dir, c)
        np.testing.assert_allclose(got['PS']['PS'].values, want['PS'] - c['era']['PS'], rtol=0, atol=2.5e-7 * float(np.max(want['PS'])),
                                   err_msg='PS_delta')          # PS itself agrees to rtol 2.5e-7 there
        level = _r_deltas(c, want['PS'])
        for var, name in zip(VARS, ('T', 'RELHUM', 'U', 'V')):
            np.testing.assert_allclose(got[name][name].values, level[var], rtol=tol4[var][0], atol=tol4[var][1], err_msg=name)
        base = _r_deltas(c, c['era']['PS'])
        assert np.abs(got['T']['T'].values - base['ta']).max() > 1e-6            # not the deltas on the ERA levels


def test_cli_interpolate_time(gpu, files):
    """-D interpolate_time: the nine files per time step, `ps` from ps_delta.nc; a lerped instant is float64, an exact hit
    keeps the file's float32; values against R.load_delta_values at rtol 1e-9; the ERA5 file's time axis."""
    from pgw4era5_amd import ncio
    s3, dbg, ctx = gpu
    root, cases, ps_delta = files
    out_dir = str(root / 'out_time')
    names = ('tos', 'tas', 'hurs', 'ps', 'ta', 'hur', 'ua', 'va', 'zg')
    res = s3._cli(['-i', str(root / 'era'), '-o', out_dir, '-d', str(root / 'deltas'), '-f', '2006080200', '-l', '2006080203',
                   '-H', '3', '-p', '1', '-D', 'interpolate_time'])
    assert len(res) == 2
    s3._cli(['-i', str(root / 'era'), '-o', out_dir, '-d', str(root / 'deltas'), '-f', '2006081512', '-l', '2006081512',
             '-H', '3', '-p', '1', '-D', 'interpolate_time'])
    stamps = ['cas{:%Y%m%d%H}0000.nc'.format(c['target_dt']) for c in cases]
    assert sorted(os.listdir(out_dir)) == sorted('delta_%s_%s' % (v, s) for v in names for s in stamps)
    for c, stamp in zip(cases, stamps):
        exact = c['target_dt'] == RECORD_STEP
        tsec = (np.datetime64(c['target_dt']).astype('datetime64[s]') - np.datetime64('1970-01-01T00:00:00')).astype(np.float64)
        for v in names:
            ds = ncio.open_dataset(os.path.join(out_dir, 'delta_%s_%s' % (v, stamp)), decode_times=False)
            src = ps_delta if v == 'ps' else c['deltas'][v]
            want = R.load_delta_values(src, c['delta_times'], c['target_dt'])
            got = ds[v].values
            assert got.dtype == (np.float32 if exact else np.float64) == want.dtype, (v, stamp)
            assert ds[v].dims == (('time', 'plev', 'lat', 'lon') if src.ndim == 4 else ('time', 'lat', 'lon'))
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, equal_nan=True, err_msg='%s %s' % (v, stamp))
            if exact:
                np.testing.assert_array_equal(got[0], src[7])
            np.testing.assert_array_equal(ds['time'].values, [tsec])
            assert ds['time'].attrs['units'] == 'seconds since 1970-01-01 00:00:00'
            if src.ndim == 4:
                np.testing.assert_array_equal(ds['plev'].values, c['plev'])
