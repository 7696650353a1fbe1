"""GPU parity tests: the HIP path (through the C-ABI) against the oracle on the same seeded
inputs, and against the golden vectors made by the reference's own leaf functions.

Tolerances: all kernels compute in fp64; outputs must agree with the fp64 oracle to 1e-6
relative (BASELINE.json north_star) - in practice the observed differences are ~1e-13 (FMA
contraction and libm-vs-ocml exp/log), so the tests assert 1e-9 where no cancellation occurs and
the north_star 1e-6 on the end-to-end fields.  Index / branch decisions (which bracket, which
level, iteration count) must be identical."""
import os

import numpy as np
import pytest

from oracle import pgw_oracle as O
from oracle import pgw_oracle_refdtype as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RT = 1e-9


@pytest.fixture(scope='module')
def F():
    from pgw4era5_amd import functions
    return functions


def _case(nlat=7, nlon=12, nlev=20, seed=0, dtype=np.float64):
    from pgw4era5_amd import synthetic
    return synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=seed, dtype=dtype)


# ------------------------------------------------------------------ golden vectors (reference)
@pytest.mark.parametrize('mode', ['constant', 'linear', 'nan'])
def test_interp_extrap_1d_golden(F, golden, mode):
    g, meta = golden
    got = F.interp_extrap_1d(g['kat_src_x'], g['kat_src_y'], g['kat_targ_x'], mode)
    np.testing.assert_allclose(got, g['kat_' + mode], rtol=1e-14, equal_nan=True)
    sx, sy, tx = g['rnd_src_x'], g['rnd_src_y'], g['rnd_targ_x']
    for c in range(sx.shape[0]):
        got = F.interp_extrap_1d(sx[c], sy[c], tx[c], mode)
        np.testing.assert_allclose(got, g['rnd_' + mode][c], rtol=1e-13, atol=1e-15, equal_nan=True, err_msg=str(c))


def test_interp_off_golden_and_error(F, golden):
    g, meta = golden
    for k, c in enumerate(g['rnd_off_cases']):
        got = F.interp_extrap_1d(g['rnd_src_x'][c], g['rnd_src_y'][c], g['rnd_targ_x_inrange'][c], 'off')
        np.testing.assert_allclose(got, g['rnd_off'][k], rtol=1e-13, atol=1e-15, equal_nan=True)
    with pytest.raises(ValueError) as e:
        F.interp_extrap_1d(g['kat_src_x'], g['kat_src_y'], g['kat_targ_x'], 'off')
    assert str(e.value) == meta['kat_off_error']
    with pytest.raises(ValueError):
        F.interp_extrap_1d(g['kat_src_x'], g['kat_src_y'], g['kat_targ_x'], 'cubic')


@pytest.mark.parametrize('mode', ['constant', 'linear', 'nan'])
def test_interp_1d_for_timelatlon_golden(F, golden, mode):
    g, meta = golden
    v, s, t = g['b4_var'], g['b4_src_lnp'], g['b4_targ_lnp']
    buf = np.zeros_like(g['b4_' + mode])
    F.interp_1d_for_timelatlon(v, s, t, buf, v.shape[0], v.shape[2], v.shape[3], mode)
    np.testing.assert_allclose(buf, g['b4_' + mode], rtol=1e-13, atol=1e-15, equal_nan=True)
    bad = s.copy(); bad[0, :, 1, 2] = bad[0, ::-1, 1, 2]
    with pytest.raises(ValueError) as e:
        F.interp_1d_for_timelatlon(v, bad, t, buf, v.shape[0], v.shape[2], v.shape[3], 'constant')
    assert str(e.value) == meta['b4_descending_error']
    assert e.value.column == 1 * v.shape[3] + 2


def test_replace_delta_sfc_golden(F, golden):
    g, meta = golden
    for i, ps in enumerate(g['rds_ps']):
        P, D = F.replace_delta_sfc(g['rds_plev'], ps, g['rds_delta'], float(g['rds_sfc']))
        np.testing.assert_array_equal(P, g['rds_out_P'][i])
        np.testing.assert_array_equal(D, g['rds_out_D'][i])
    for ps in meta['rds_errors']:
        with pytest.raises(ValueError):
            F.replace_delta_sfc(g['rds_plev'], float(ps), g['rds_delta'], 9.25)


def test_humidity_golden(F, golden):
    g, _ = golden
    ta, pa, q = g['hum_ta'], g['hum_pa'], g['hum_hus']
    T0, Ti = 273.16, 250.16
    a = np.where(ta >= T0, 1.0, np.where(ta <= Ti, 0.0, ((ta - Ti) / (T0 - Ti)) ** 2))
    es = a * g['hum_esat_water'] + (1 - a) * g['hum_esat_ice']          # reference leaf values
    rh = F.specific_to_relative_humidity(q, pa, ta)
    np.testing.assert_allclose(rh, g['hum_e'] / es * 100, rtol=1e-13)
    q2 = F.relative_to_specific_humidity(rh, pa, ta)
    ok = pa > 10 * g['hum_e']
    np.testing.assert_allclose(q2[ok], q[ok], rtol=1e-11, atol=1e-18)
    # the leaf helpers of functions.py:58-105 under their own names, against the reference's values
    np.testing.assert_array_equal(F.specific_humidity_to_vapor_pressure(q, pa), g['hum_e'])          # arithmetic only: same bits
    np.testing.assert_array_equal(F.vapor_pressure_to_specific_humidity(g['hum_e'], pa), g['hum_q_from_e'])
    np.testing.assert_allclose(F.saturation_vapor_pressure_water_or_ice(pa, ta, water=True), g['hum_esat_water'], rtol=1e-14)
    np.testing.assert_allclose(F.saturation_vapor_pressure_water_or_ice(pa, ta, water=False), g['hum_esat_ice'], rtol=1e-14)
    np.testing.assert_allclose(F.saturation_vapor_pressure_water_and_ice(pa, ta), es, rtol=1e-14)
    import datetime as _dt
    assert F.dt64_to_dt(np.datetime64('2006-08-02T03:00:00')) == _dt.datetime(2006, 8, 2, 3, 0, 0)


def test_integrate_tos_golden(F, golden):
    g, _ = golden
    got = F.integrate_tos(g['tos_tos'], g['tos_ts'], g['tos_land'], g['tos_ice'])
    np.testing.assert_allclose(got, g['tos_out'], rtol=1e-15, equal_nan=True)


# ------------------------------------------------------------------ oracle, seeded inputs
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_pressure_and_humidity_vs_oracle(F, dtype):
    c = _case(dtype=dtype, seed=3)
    era = c['era']
    pa_hl, pa = F.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    o_hl, o_pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'].astype(np.float64))
    tol = 1e-13 if dtype == np.float64 else 1e-6
    np.testing.assert_allclose(pa_hl, o_hl, rtol=tol, atol=1e-30)
    np.testing.assert_allclose(pa, o_pa, rtol=tol)
    rh = F.specific_to_relative_humidity(era['QV'], pa, era['T'])
    o_rh = O.specific_to_relative_humidity(era['QV'].astype(np.float64), pa.astype(np.float64), era['T'].astype(np.float64))
    np.testing.assert_allclose(rh, o_rh, rtol=1e-12 if dtype == np.float64 else 1e-6)
    q = F.relative_to_specific_humidity(rh, pa, era['T'])
    o_q = O.relative_to_specific_humidity(rh.astype(np.float64), pa.astype(np.float64), era['T'].astype(np.float64))
    np.testing.assert_allclose(q, o_q, rtol=1e-12 if dtype == np.float64 else 1e-6)


@pytest.mark.parametrize('shape', [(7, 12, 20), (5, 9, 33), (1, 1, 4)])
@pytest.mark.parametrize('full', [True, False])
def test_integ_geopot_vs_oracle(F, shape, full):
    nlat, nlon, nlev = shape
    c = _case(nlat, nlon, nlev, seed=4)
    era = c['era']
    pa_hl, _ = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    lvl1 = np.arange(1, nlev + 2)
    for p_ref in (30000.0, 50000.0):
        want = O.integ_geopot(pa_hl, era['FIS'], era['T'], era['QV'], lvl1, p_ref)
        got = F.integ_geopot(pa_hl, era['FIS'], era['T'], era['QV'], lvl1, p_ref, full_column=full)
        np.testing.assert_allclose(got, want, rtol=RT)
    pf = np.where(era['PS'] > 90000, 70000.0, 30000.0)
    want = O.integ_geopot(pa_hl, era['FIS'], era['T'], era['QV'], lvl1, pf)
    got = F.integ_geopot(pa_hl, era['FIS'], era['T'], era['QV'], lvl1, pf, full_column=full)
    np.testing.assert_allclose(got, want, rtol=RT)


def test_integ_geopot_isothermal_exact_and_errors(F):
    c = _case(6, 8, 30, seed=5)
    era = c['era']
    pa_hl, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    T = np.full(pa.shape, 250.0); q = np.zeros(pa.shape)
    got = F.integ_geopot(pa_hl, era['FIS'], T, q, np.arange(1, 32), 30000.0)
    np.testing.assert_allclose(got, era['FIS'] + O.CON_RD * 250.0 * np.log(era['PS'] / 30000.0), rtol=1e-12)
    with pytest.raises(ValueError) as e:
        F.integ_geopot(pa_hl, era['FIS'], T, q, np.arange(1, 32), 200000.0)
    assert 'p_ref locally lies below the surface' in str(e.value)
    with pytest.raises(KeyError):
        F.integ_geopot(pa_hl, era['FIS'], T, q, np.arange(1, 32), 1e-5)   # only the top half level matches
    # non-monotone column: the reference's nanargmin rule, not "first crossing"
    p2 = pa_hl.copy(); p2[0, 10, 2, 3] = 95000.0
    want = O.integ_geopot(p2, era['FIS'], T, q, np.arange(1, 32), 30000.0)
    got = F.integ_geopot(p2, era['FIS'], T, q, np.arange(1, 32), 30000.0)
    np.testing.assert_allclose(got, want, rtol=RT)
    # NaN pressure is replaced by 1e-4 like pa_hl.where(pa_hl > 0, 0.0001)
    p3 = pa_hl.copy(); p3[0, 3, 1, 1] = np.nan
    np.testing.assert_allclose(F.integ_geopot(p3, era['FIS'], T, q, np.arange(1, 32), 30000.0),
                               O.integ_geopot(p3, era['FIS'], T, q, np.arange(1, 32), 30000.0), rtol=RT)


@pytest.mark.parametrize('mode', ['off', 'linear', 'constant', 'nan'])
@pytest.mark.parametrize('S,N', [(19, 20), (34, 41), (2, 3), (70, 9)])
def test_interp_logp_4d_vs_oracle(F, mode, S, N):
    rng = np.random.default_rng(S * 100 + N)
    nt, nlat, nlon = 2, 5, 13
    ps = np.sort(rng.uniform(100, 1e5, (nt, S, nlat, nlon)), axis=1)
    lo, hi = (ps.min(1, keepdims=True), ps.max(1, keepdims=True)) if mode == 'off' else (50.0, 1.05e5)
    pt = np.sort(rng.uniform(lo, hi, (nt, N, nlat, nlon)), axis=1)
    v = rng.normal(0, 3, ps.shape)
    v[0, 1, 2, 3] = np.nan
    if mode != 'off':
        pt[1, 0, 0, 0] = ps[1, 0, 0, 0]            # exact hit on the first source level
        pt[1, :, 0, 0] = np.sort(pt[1, :, 0, 0])
        pt[0, :, 4, 4] = pt[0, ::-1, 4, 4].copy()  # descending target column: error in the reference
    if mode == 'off' or True:
        try:
            want = O.interp_logp_4d(v, ps, pt, mode)
            err = None
        except ValueError as e:
            want, err = None, str(e)
    if err is not None:
        with pytest.raises(ValueError) as e:
            F.interp_logp_4d(v, ps, pt, mode)
        assert str(e.value) == err
        pt[0, :, 4, 4] = np.sort(pt[0, :, 4, 4])
        want = O.interp_logp_4d(v, ps, pt, mode)
    got = F.interp_logp_4d(v, ps, pt, mode)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize('mode', ['linear', 'constant', 'nan'])
def test_interp_logp_unsorted_targets_and_nans(F, mode):
    """Targets that are not monotone inside a column (legal as long as first <= last: the reference scans the
    source from the start for every target, functions.py:527-548), NaN targets and NaN source pressures."""
    rng = np.random.default_rng(77)
    nt, S, N, nlat, nlon = 1, 11, 29, 4, 37
    ps = np.sort(rng.uniform(100, 1e5, (nt, S, nlat, nlon)), axis=1)
    pt = rng.uniform(50, 1.05e5, (nt, N, nlat, nlon))
    pt[:, 0] = 60.0; pt[:, -1] = 1.04e5                      # first <= last everywhere, shuffled in between
    pt[0, 5, 1, 2] = np.nan
    pt[0, 6, 1, 2] = 300.0
    ps[0, 4, 2, 3] = np.nan                                  # a NaN source level is never selected as upper bracket
    pt[0, 1:, 3, 5] = ps[0, [0, 3, 10] * 9 + [10], 3, 5]     # exact hits incl. first / last source level
    v = rng.normal(0, 3, ps.shape)
    want = O.interp_logp_4d(v, ps, pt, mode)
    got = F.interp_logp_4d(v, ps, pt, mode)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12, equal_nan=True)
    # float32 storage, pre-computed logs (interp_1d_for_timelatlon signature)
    buf = np.zeros(pt.shape)
    ok = np.isfinite(ps).all(axis=1) & np.isfinite(pt).all(axis=1)
    lps, lpt = np.log(np.where(ok[:, None], ps, 1.0)), np.log(np.where(ok[:, None], pt, 1.0))
    F.interp_1d_for_timelatlon(v, lps, lpt, buf, nt, nlat, nlon, mode)
    want2 = np.zeros(pt.shape)
    O.interp_1d_for_timelatlon(v, lps, lpt, want2, nt, nlat, nlon, mode)
    np.testing.assert_allclose(buf, want2, rtol=1e-12, atol=1e-13, equal_nan=True)


def test_interp_shape_errors(F):
    a = np.ones((1, 3, 2, 2))
    with pytest.raises(ValueError) as e:
        F.interp_logp_4d(a, np.ones((2, 3, 2, 2)), a)
    assert str(e.value) == 'Time dimension of input files is inconsistent!'
    with pytest.raises(ValueError) as e:
        F.interp_logp_4d(a, a, np.ones((1, 3, 3, 2)))
    assert str(e.value) == 'Lat dimension of input files is inconsistent!'
    with pytest.raises(ValueError) as e:
        F.interp_logp_4d(a, a, np.ones((1, 3, 2, 5)))
    assert str(e.value) == 'Lon dimension of input files is inconsistent!'


@pytest.mark.parametrize('with_sfc', [True, False])
def test_vert_interp_delta_vs_oracle(F, with_sfc):
    c = _case(9, 11, 25, seed=6)
    era, d = c['era'], c['deltas']
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    delta = d['ta'][3:4]
    dsfc = d['tas'][3:4] if with_sfc else None
    psh = d['ps_hist'][3:4].copy() if with_sfc else None
    if with_sfc:
        psh[0, 0, 0] = 101000.0        # above max(plev): only the last level is replaced
        psh[0, 0, 1] = 85000.0         # exactly a plev: k = index below it
        psh[0, 0, 2] = 60000.0001
    with pytest.raises(ValueError) as e:
        F.vert_interp_delta(delta, pa, dsfc, psh, plev=c['plev'])
    assert 'ERA5 top pressure is lower than climate delta top pressure' in str(e.value)
    want = O.vert_interp_delta(delta, c['plev'], pa, dsfc, psh, ignore_top_pressure_error=True)
    got = F.vert_interp_delta(delta, pa, dsfc, psh, ignore_top_pressure_error=True, plev=c['plev'])
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-13)
    if with_sfc:
        psh[0, 2, 2] = 50.0            # above the delta top -> bare ValueError()
        with pytest.raises(ValueError) as e:
            F.vert_interp_delta(delta, pa, dsfc, psh, ignore_top_pressure_error=True, plev=c['plev'])
        assert str(e.value) == ''


def _single_column_top_inputs():
    """(plev, delta, delta_sfc, ps_hist, [(target_P, raises), ...]) of test_top_pressure_check_sees_a_single_column:
    1 time step, 5 x 13 = 65 columns (one block; the second wave has one live lane, column 64), N = 4 target levels."""
    rng = np.random.default_rng(417)
    plev = np.array([100000.0, 85000.0, 50000.0, 20000.0, 10000.0])          # file order; min(plev) = 10000
    delta = rng.normal(size=(1, plev.size, 5, 13))
    dsfc = rng.normal(size=(1, 5, 13))
    psh = rng.uniform(90000.0, 99000.0, size=(1, 5, 13))
    ok = np.sort(rng.uniform(10000.5, 101000.0, size=(1, 4, 5, 13)), axis=1)   # every level >= min(plev)
    below = np.nextafter(plev.min(), 0.0)                                       # one ulp below min(plev)
    inputs = []
    for col, top, raises in [(64, below, True), (0, below, True), (64, plev.min(), False)]:
        pa = ok.copy()
        pa.reshape(4, 65)[0, col] = top
        assert (pa.reshape(4, 65)[0] < plev.min()).sum() == (1 if raises else 0)
        inputs.append((pa, raises))
    return plev, delta, dsfc, psh, inputs


def test_top_pressure_check_sees_a_single_column(F):
    """The top-pressure check (functions.py:417-420) decided by ONE column: every target pressure >= min(plev) except the
    top level of the last column of the block (the single live lane of the second wave), or of the first, one ulp below it
    -> the reference's ValueError; exactly equal -> none (the comparison is strict).  The oracle must decide each input the
    same way.  Then the file paths that carry the check (quad kernel, pair kernels, i_reinterp): all raise without -t,
    all return with it."""
    plev, delta, dsfc, psh, inputs = _single_column_top_inputs()
    msg = 'ERA5 top pressure is lower than climate delta top pressure'
    for sfc in [(dsfc, psh), (None, None)]:
        for pa, raises in inputs:
            if raises:
                with pytest.raises(ValueError) as e:
                    O.vert_interp_delta(delta, plev, pa, *sfc, ignore_top_pressure_error=False)
                assert msg in str(e.value)
                with pytest.raises(ValueError) as e:
                    F.vert_interp_delta(delta, pa, *sfc, ignore_top_pressure_error=False, plev=plev)
                assert msg in str(e.value)
            else:
                want = O.vert_interp_delta(delta, plev, pa, *sfc, ignore_top_pressure_error=False)
                got = F.vert_interp_delta(delta, pa, *sfc, ignore_top_pressure_error=False, plev=plev)
                np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-13)
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    c = _case(8, 12, 27, seed=81)                                  # model top above the delta top
    args = (c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'])
    with pytest.raises(ValueError) as e:
        O.pgw_for_era5_arrays(*args, ignore_top_pressure_error=False)
    assert msg in str(e.value)
    for opts, kw in [({}, {}), (dict(quad=0), {}), ({}, dict(i_reinterp=True))]:
        old = {k: ctx.set_option(k, v) for k, v in opts.items()}
        try:
            with pytest.raises(ValueError) as e:
                s3.pgw_for_era5_arrays(*args, ignore_top_pressure_error=False, **kw)
            assert msg in str(e.value), (opts, kw)
            out = s3.pgw_for_era5_arrays(*args, ignore_top_pressure_error=True, **kw)
            assert np.isfinite(out['PS']).all() and out['n_iter'] >= 1, (opts, kw)
        finally:
            for k, v in old.items():
                ctx.set_option(k, v)


def test_time_lerp_vs_oracle(F):
    rng = np.random.default_rng(8)
    b, a = rng.normal(size=(3, 4, 5)), rng.normal(size=(3, 4, 5))
    tb, ta, t = np.datetime64('2006-07-15T12:00:00'), np.datetime64('2006-08-15T12:00:00'), np.datetime64('2006-08-02T03:00:00')
    want = O.time_lerp(b, a, tb, ta, t)
    ns = 'datetime64[ns]'
    x_hi = float((ta.astype(ns) - tb.astype(ns)).astype(np.int64)); x_new = float((t.astype(ns) - tb.astype(ns)).astype(np.int64))
    np.testing.assert_array_equal(F.time_lerp(b, a, x_hi, x_new), want)      # same operation order, no FMA contraction


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_adjust_ps_loop_vs_oracle(F, dtype):
    c = _case(8, 12, 30, seed=7, dtype=dtype)
    era, d = c['era'], c['deltas']
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    akm, bkm = O.full_level_coeffs(era['ak'], era['bk'])
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], f64(era['PS']))
    ta_pgw = (f64(era['T']) + 2.0).astype(dtype)
    hur = O.specific_to_relative_humidity(f64(era['QV']), pa, f64(era['T']))
    hur_pgw = (hur - 1.0).astype(dtype)
    dzg = d['zg'][6, 7][None]                 # 300 hPa
    want = O.adjust_ps_loop(era['ak'], era['bk'], akm, bkm, f64(era['PS']), f64(era['FIS']), f64(era['T']), f64(era['QV']),
                            f64(ta_pgw), f64(hur_pgw), f64(dzg))
    got = F.adjust_ps_loop(era['ak'], era['bk'], era['PS'], era['FIS'], era['T'], era['QV'], ta_pgw, hur_pgw, dzg)
    assert got['n_iter'] == want['n_iter']
    np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=1e-6, atol=1e-9)
    tol = 1e-10 if dtype == np.float64 else 1e-6
    np.testing.assert_allclose(got['ps_pgw'], want['ps_pgw'], rtol=tol)
    np.testing.assert_allclose(got['hus_pgw'], want['hus_pgw'], rtol=tol)


def test_adjust_ps_loop_not_converged(F):
    c = _case(4, 4, 12, seed=9)
    era, d = c['era'], c['deltas']
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    hur = O.specific_to_relative_humidity(era['QV'], pa, era['T'])
    with pytest.raises(ValueError) as e:
        F.adjust_ps_loop(era['ak'], era['bk'], era['PS'], era['FIS'], era['T'], era['QV'], era['T'] + 2, hur,
                         d['zg'][6, 7][None], max_n_iter=3)
    assert 'did not converge' in str(e.value)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_whole_file_vs_oracle(dtype):
    from pgw4era5_amd import step_03_apply_to_era as s3
    c = _case(10, 10, 20, seed=0, dtype=dtype)          # BASELINE.json configs[0] shape
    # float32 storage here in the 'fast' mode (float64 arithmetic on the stored values); the reference-dtype mode has
    # its own tests below (test_reference_dtype_mode_*)
    got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, ref_dtype=False)
    era64 = {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v)
             for k, v in c['era'].items()}
    d64 = {k: np.asarray(v, dtype=np.float64) for k, v in c['deltas'].items()}
    want = O.pgw_for_era5_arrays(era64, d64, c['delta_times'], c['plev'], c['target_dt'], True)
    assert got['n_iter'] == want['n_iter']
    tol = 1e-9 if dtype == np.float64 else 1e-6
    for k in ['PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE', 'RELHUM_pgw']:
        rtol = tol
        if dtype == np.float32 and k == 'QV':
            # f32 STORAGE of the intermediate ta_pgw: e_sat(T) amplifies T's f32 rounding
            # (1.5e-5 K at 215 K) by d ln(e_sat)/dT = 0.13 /K -> 2e-6 relative at the cold top
            rtol = 3e-6
        np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=1e-5 if (dtype == np.float32 and k in ('U', 'V', 'RELHUM_pgw')) else 1e-12,
                                   equal_nan=True, err_msg=k)
    # the converged state satisfies the loop's criterion when re-evaluated by the standalone oracle
    assert want['max_err'][-1] <= 0.15


def test_regrid_vs_oracle(F):
    from pgw4era5_amd import synthetic
    g = synthetic.make_gcm_grid_case(seed=2)
    g['field'][1, 2, 5, 7] = np.nan
    want = O.regrid_lat_lon(g['field'], g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon'])
    got = F.regrid_field(g['field'], g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon'])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14, equal_nan=True)
    assert np.isnan(got).sum() == np.isnan(want).sum() > 0
    with pytest.raises(ValueError):
        F.regrid_field(g['field'][..., ::-1, :], g['src_lat'][::-1], g['src_lon'], g['targ_lat'], g['targ_lon'])
    with pytest.raises(ValueError):
        F.regrid_field(g['field'][..., :40], g['src_lat'], g['src_lon'][:40], g['targ_lat'], g['targ_lon'])
    # -180..180 target on a 0..360 source (periodic extension to the west)
    tl = g['targ_lon'] - 180.0
    want = O.regrid_lat_lon(g['field'], g['src_lat'], g['src_lon'], g['targ_lat'], tl)
    got = F.regrid_field(g['field'], g['src_lat'], g['src_lon'], g['targ_lat'], tl)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14, equal_nan=True)


@pytest.mark.parametrize('case', ['fine_multi_block', 'coarse_target', 'unsorted_lons', 'f32'])
def test_regrid_block_window_paths(F, case):
    """The regridding kernel stages the latitude pass of a block's source-column window in LDS; cover several
    blocks per row with a ragged last one and the periodic wrap inside a block (fine target), windows wider than
    the LDS tile (target coarser than the source -> direct gathers), target longitudes in arbitrary order, and
    float32 storage - all against the oracle."""
    from pgw4era5_amd import synthetic
    if case == 'fine_multi_block':
        g = synthetic.make_gcm_grid_case(nlat_src=24, nlon_src=48, nlat=19, nlon=700, nplev=2, ntime=3, seed=5)
        g['targ_lon'] = g['targ_lon'] - 123.4                      # wrap somewhere inside a block
    elif case == 'coarse_target':
        g = synthetic.make_gcm_grid_case(nlat_src=40, nlon_src=1200, nlat=13, nlon=300, nplev=2, ntime=2, seed=6)
    elif case == 'unsorted_lons':
        g = synthetic.make_gcm_grid_case(nlat_src=24, nlon_src=60, nlat=11, nlon=333, nplev=3, ntime=1, seed=7)
        g['targ_lon'] = np.random.default_rng(0).permutation(g['targ_lon'])
    else:
        g = synthetic.make_gcm_grid_case(nlat_src=30, nlon_src=64, nlat=21, nlon=515, nplev=3, ntime=2, seed=8, dtype=np.float32)
    g['field'][0, 1, 3, 5] = np.nan
    want = O.regrid_lat_lon(g['field'].astype(np.float64), g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon'])
    got = F.regrid_field(g['field'], g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon'])
    assert got.dtype == g['field'].dtype
    tol = dict(rtol=1e-12, atol=1e-14) if case != 'f32' else dict(rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got, want, equal_nan=True, **tol)
    assert np.isnan(got).sum() == np.isnan(want).sum()
    assert np.isnan(want).sum() > 0 or case in ('coarse_target', 'unsorted_lons')     # a coarse target may miss the NaN cell


def test_regrid_full_size_config4_properties_and_band(F):
    """BASELINE.json configs[3] at full size: one 19-level variable x 12 months from an MPI-ESM1-2-HR-like 192 x 384
    Gaussian grid (lats short of the poles, lon 0 ... 359.0625) to the ERA5 0.25 deg grid (721 x 1440), through
    regrid_field on the GPU.  The oracle needs minutes for 237 M outputs, so the full result is checked through
    size-independent properties (functions.py:817-893) and a 6-row band of it against the oracle."""
    from pgw4era5_amd import synthetic
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    g = synthetic.make_gcm_grid_case(nlat_src=192, nlon_src=384, nlat=721, nlon=1440, nplev=19, ntime=12, seed=4)
    f, slat, slon, tlat, tlon = g['field'], g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon']
    nt, npl = f.shape[:2]
    # plane (0,0): zonally constant (depends on latitude only); (0,1): linear in latitude; (0,2): linear in longitude;
    # (0,3): one NaN cell; the rest random
    f[0, 0] = np.sin(np.deg2rad(slat))[:, None] * np.ones(len(slon))
    f[0, 1] = (2.0 + 0.25 * slat)[:, None] * np.ones(len(slon))
    f[0, 2] = np.ones(len(slat))[:, None] * (1.0 + 0.125 * slon)[None, :]
    f[0, 3, 100, 200] = np.nan
    d_src = ctx.to_device(f)
    d_out = F.regrid_field(d_src, slat, slon, tlat, tlon)
    got = d_out.numpy()
    d_src.free(); d_out.free()
    assert got.shape == (nt, npl, 721, 1440)
    # --- zonally constant in, zonally constant out, equal to the 1-D latitude interpolation (pole rows: the zonal mean
    # of the nearest source row = the row's own constant)
    zc = got[0, 0]
    assert np.ptp(zc, axis=1).max() == 0.0
    lat_ext = np.concatenate([[-90.0], slat, [90.0]])
    col_ext = np.concatenate([[f[0, 0, 0, 0]], f[0, 0, :, 0], [f[0, 0, -1, 0]]])
    np.testing.assert_allclose(zc[:, 0], O.interp1d_linear(lat_ext, col_ext, tlat, axis=0), rtol=1e-14, atol=1e-15)
    # --- linear in latitude: exact inside the source latitudes; beyond them the pole row (zonal mean of the last row)
    # makes it constant (functions.py:833-842)
    inside = (tlat >= slat[0]) & (tlat <= slat[-1])
    np.testing.assert_allclose(got[0, 1][inside], (2.0 + 0.25 * tlat[inside])[:, None] * np.ones(1440), rtol=1e-13)
    np.testing.assert_allclose(got[0, 1][tlat > slat[-1]], 2.0 + 0.25 * slat[-1], rtol=1e-13)
    np.testing.assert_allclose(got[0, 1][tlat < slat[0]], 2.0 + 0.25 * slat[0], rtol=1e-13)
    # --- linear in longitude: exact up to the last source longitude; in the periodic gap 359.0625 ... 360 the copy at
    # lon + 360 closes the circle (functions.py:866-874): interpolation between the last and the first source column
    # (rows between the last source latitude and the pole blend towards the pole row's zonal mean: `inside` rows only)
    lin = got[0, 2][inside]
    west = tlon <= slon[-1]
    np.testing.assert_allclose(lin[:, west], np.ones(len(lin))[:, None] * (1.0 + 0.125 * tlon[west])[None, :], rtol=1e-13)
    gap = ~west
    assert gap.sum() == 3                                   # 359.25, 359.5, 359.75
    y_last, y_first = 1.0 + 0.125 * slon[-1], 1.0 + 0.125 * slon[0]
    want_gap = (y_first - y_last) / ((slon[0] + 360) - slon[-1]) * (tlon[gap] - slon[-1]) + y_last
    np.testing.assert_allclose(lin[:, gap], np.ones(len(lin))[:, None] * want_gap[None, :], rtol=1e-13)
    # --- pole rows of every plane: the zonal mean (NaN-skipping) of the first / last source row, on every longitude
    rnd = got[5, 7]
    np.testing.assert_allclose(rnd[0], np.full(1440, f[5, 7, 0].mean()), rtol=1e-13)
    np.testing.assert_allclose(rnd[-1], np.full(1440, f[5, 7, -1].mean()), rtol=1e-13)
    # --- NaN propagation: exactly the targets whose 2 x 2 stencil touches source cell (100, 200)
    nanmask = np.isnan(got[0, 3])
    jj = np.nonzero((tlat > slat[99]) & (tlat < slat[101]))[0]
    ii = np.nonzero((tlon > slon[199]) & (tlon < slon[201]))[0]
    want_mask = np.zeros_like(nanmask)
    want_mask[np.ix_(jj, ii)] = True
    np.testing.assert_array_equal(nanmask, want_mask)
    assert not np.isnan(np.delete(got.reshape(nt * npl, 721, 1440), 3, axis=0)).any()
    # --- a 6-row band (both pole rows, two rows around the equator, two mid-latitude rows) of all 228 planes vs the oracle
    rows = np.array([0, 1, 360, 361, 612, 720])
    want = O.regrid_lat_lon(f, slat, slon, tlat[rows], tlon)
    np.testing.assert_allclose(got[:, :, rows], want, rtol=1e-12, atol=1e-14, equal_nan=True)


class FakeDataArray:
    """Stand-in for xarray.DataArray (not installable here): `.values/.dims/.coords/.shape/.dtype`, `.copy(data=)`,
    `.transpose(*dims)`, `.isel`, `len()` - what the reference's step_03 lines touch on the results of the functions
    below.  NOT an ncio.Field: no `.like`, so operands.out_like must take the `.copy(data=)` route."""

    def __init__(self, values, dims, coords=None):
        self.values = np.asarray(values)
        self.dims = tuple(dims)
        self.coords = dict(coords or {})
        assert self.values.ndim == len(self.dims)

    shape = property(lambda self: self.values.shape)
    dtype = property(lambda self: self.values.dtype)

    def __len__(self):
        return self.values.shape[0]

    def copy(self, deep=True, data=None):
        v = self.values.copy() if data is None else np.asarray(data)
        if v.shape != self.values.shape:
            raise ValueError('replacement data must match the shape')
        return FakeDataArray(v, self.dims, self.coords)

    def transpose(self, *dims):
        return FakeDataArray(self.values.transpose([self.dims.index(d) for d in dims]), dims, self.coords)


def test_functions_rewrap_xarray_like_inputs(F):
    """INTEGRATION.md section A (import swap): the reference's own call sequence on labelled arrays that are not this
    package's Field - step_03_apply_to_era.py:87-94 (RELHUM of the ERA state followed by `.transpose(dim names)`),
    :262-287 (hus_pgw, integ_geopot of both states with `era_file[HLEV_ERA]` as level1) - returns labelled arrays
    with the inputs' dims / coords, and operands given in another dimension order are aligned by NAME."""
    c = _case(5, 7, 12, seed=3)
    era = c['era']
    d4, d4h, d3 = ('time', 'level', 'lat', 'lon'), ('time', 'level1', 'lat', 'lon'), ('time', 'lat', 'lon')
    coords = dict(lat=c['lat'], lon=c['lon'])
    W = lambda v, dims: FakeDataArray(v, dims, coords)
    pa_hl_np, pa_np = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    hus, ta, pa, pa_hl = W(era['QV'], d4), W(era['T'], d4), W(pa_np, d4), W(pa_hl_np, d4h)
    # :91-94  era_file[hur] = specific_to_relative_humidity(hus, pa_era, ta).transpose(TIME_ERA, LEV_ERA, LAT_ERA, LON_ERA)
    hur = F.specific_to_relative_humidity(hus, pa, ta).transpose('time', 'level', 'lat', 'lon')
    assert isinstance(hur, FakeDataArray) and hur.dims == d4 and hur.coords['lat'] is coords['lat']
    want = O.specific_to_relative_humidity(era['QV'], pa_np, era['T'])
    np.testing.assert_allclose(hur.values, want, rtol=1e-12)
    # operands in another dimension order: xarray would align them by name
    pa_t = pa.transpose('time', 'lat', 'lon', 'level')
    hur2 = F.specific_to_relative_humidity(hus, pa_t, ta)
    np.testing.assert_array_equal(hur2.values, hur.values)
    # :262-266
    q = F.relative_to_specific_humidity(hur, pa, ta)
    assert isinstance(q, FakeDataArray) and q.dims == d4
    np.testing.assert_allclose(q.values, era['QV'], rtol=1e-9, atol=1e-18)
    # :269-287  integ_geopot(pa_hl, zgs, ta, hus, era_file[HLEV_ERA], p_ref) -> (time, lat, lon) labelled like zgs
    level1 = FakeDataArray(era['level1'], ('level1',))
    phi = F.integ_geopot(pa_hl, W(era['FIS'], d3), ta, q, level1, 30000)
    assert isinstance(phi, FakeDataArray) and phi.dims == d3 and phi.shape == era['FIS'].shape
    np.testing.assert_allclose(phi.values, O.integ_geopot(pa_hl_np, era['FIS'], era['T'], q.values, era['level1'], 30000), rtol=1e-12)
    # interp_logp_4d returns the target's labels (functions.py:472 xr.zeros_like(targ_P))
    out = F.interp_logp_4d(ta, pa, W(pa_np * 1.001, d4), extrapolate='constant')
    assert isinstance(out, FakeDataArray) and out.dims == d4
    # plain ndarrays still come back as ndarrays
    assert isinstance(F.specific_to_relative_humidity(era['QV'], pa_np, era['T']), np.ndarray)


@pytest.mark.parametrize('entry', ['pgw_test_log', 'pgw_test_log_table'])
def test_device_log_accuracy(entry):
    """pgw_log (fdlibm kernel) and pgw_log_tab (the table-driven logarithm of the hybrid-level loops) against numpy: at
    most 1 ulp from np.log on positive normal numbers, IEEE special cases through the ocml fallback.  This bounds the
    distance to numpy, not the error: np.log is itself up to 0.52 ulp off, and pgw_log_tab is up to 1.49 ulp from the
    exact logarithm while passing here (tests/test_device_math_hip.py holds both to the exact value)."""
    import ctypes as C
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    test_log = getattr(ctx.lib, entry)
    rng = np.random.default_rng(11)
    x = np.concatenate([
        rng.uniform(1e-4, 1.1e5, 200000),                       # pressures of the path
        np.exp(rng.uniform(-700, 700, 100000)),                 # all magnitudes
        1.0 + rng.uniform(-1e-3, 1e-3, 50000),                  # near 1 (cancellation-prone)
        np.array([1.0, 2.0, 0.5, np.sqrt(0.5), np.nextafter(np.sqrt(0.5), 0), 1e-4, 30000.0, 101325.0,
                  2.2250738585072014e-308, 1.7976931348623157e308]),
    ])
    d_in = ctx.to_device(x, np.float64)
    d_out = ctx.empty(x.shape, np.float64)
    ctx._check(test_log(ctx.handle, x.size, d_in.ptr, d_out.ptr))
    got, want = d_out.numpy(), np.log(x)
    ulp = np.abs(got - want) / np.spacing(np.abs(want) + 1e-300)
    assert ulp.max() <= 1.0, (ulp.max(), x[ulp.argmax()])
    assert (ulp > 0).mean() < 0.3                               # most values are bit-identical to numpy
    sp = np.array([0.0, -1.0, np.inf, np.nan, 5e-324, 1e-310])
    d_in = ctx.to_device(sp, np.float64); d_out = ctx.empty(sp.shape, np.float64)
    ctx._check(test_log(ctx.handle, sp.size, d_in.ptr, d_out.ptr))
    got = d_out.numpy()
    with np.errstate(all='ignore'):
        want = np.log(sp)
    assert got[0] == -np.inf and np.isnan(got[1]) and got[2] == np.inf and np.isnan(got[3])
    np.testing.assert_allclose(got[4:], want[4:], rtol=1e-15)


# ------------------------------------------------------------------ full size (BASELINE configs[1])
@pytest.fixture(scope='module')
def full_case():
    """One synthetic 0.25 deg L137 file on the device (fp64), processed once."""
    from pgw4era5_amd import synthetic, step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    case = synthetic.make_case(nlat=721, nlon=1440, nlev=137, seed=1, dtype=np.float64)
    deltas = s3.DeltaSet(ctx, case['deltas'], case['delta_times'], case['plev'], np.float64)
    era = s3._upload_era(ctx, case['era'], np.float64)
    coeffs = dict(ak=case['era']['ak'], bk=case['era']['bk'], soil1=case['era']['soil1'])
    out, info = s3.process_file_device(ctx, era, coeffs, deltas, case['target_dt'], True, keep_hur=True)
    return ctx, case, era, out, info


def test_full_size_band_matches_oracle(full_case):
    """A latitude band of the 1440x721 L137 file against the oracle run on that band only
    (columns are independent; the iteration count is global, so the band is compared with the
    oracle forced to the same number of passes)."""
    ctx, case, era, out, info = full_case
    rows = slice(300, 306)
    f64 = np.float64
    e = {k: (np.ascontiguousarray(v[..., rows, :], dtype=f64) if isinstance(v, np.ndarray) and v.ndim >= 3 else v)
         for k, v in case['era'].items()}
    d = {k: np.ascontiguousarray(v[..., rows, :], dtype=f64) for k, v in case['deltas'].items()}
    # oracle with the loop driven for exactly info['n_iter'] passes
    akm, bkm = O.full_level_coeffs(e['ak'], e['bk'])
    _, pa = O.hybrid_pressure(e['ak'], e['bk'], e['PS'], akm, bkm)
    relhum = O.specific_to_relative_humidity(e['QV'], pa, e['T'])
    ld = lambda k: O.load_delta_values(d[k], case['delta_times'], case['target_dt'])
    ta = e['T'] + O.vert_interp_delta(ld('ta'), case['plev'], pa, ld('tas'), ld('ps_hist'), True)
    hur = relhum + O.vert_interp_delta(ld('hur'), case['plev'], pa, ld('hurs'), ld('ps_hist'), True)
    ua = e['U'] + O.vert_interp_delta(ld('ua'), case['plev'], pa, None, None, True)
    kref = int(np.nonzero(case['plev'] == 30000.0)[0][0])
    # drive the oracle loop manually for n_iter passes
    dps = np.zeros_like(e['PS']); adj = np.zeros_like(e['PS'])
    lvl1 = np.arange(1, len(e['ak']) + 1)
    pa_hl_era, _ = O.hybrid_pressure(e['ak'], e['bk'], e['PS'], akm, bkm)
    phi_era = O.integ_geopot(pa_hl_era, e['FIS'], e['T'], e['QV'], lvl1, 30000.0)
    for _ in range(info['n_iter']):
        dps = dps + adj
        ps = e['PS'] + dps
        pa_hl_p, pa_p = O.hybrid_pressure(e['ak'], e['bk'], ps, akm, bkm)
        hus = O.relative_to_specific_humidity(hur, pa_p, ta)
        err = (O.integ_geopot(pa_hl_p, e['FIS'], ta, hus, lvl1, 30000.0) - phi_era) - ld('zg')[:, kref] * O.CON_G
        adj = -0.95 * ps / (O.CON_RD * ta[:, -1]) * err
    for name, want in (('PS', ps), ('T', ta), ('QV', hus), ('U', ua), ('_hur_pgw', hur)):
        got = out[name].numpy()[..., rows, :]
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 if name in ('U', '_hur_pgw') else 1e-14, err_msg=name)
    assert np.abs(err).max() <= info['max_err'][-1] * (1 + 1e-9) <= 0.15


def test_full_size_converged_state_is_hydrostatically_consistent(full_case):
    """Size-independent property: re-evaluating the loop's criterion on the full 0.25 deg L137
    output with the STANDALONE signature-faithful kernels (pressure_levels, integ_geopot,
    relative_to_specific_humidity) reproduces the loop's last max|err| <= 0.15."""
    from pgw4era5_amd import functions as F
    ctx, case, era, out, info = full_case
    assert 2 <= info['n_iter'] <= 19 and info['max_err'][-1] <= 0.15 < info['max_err'][-2]
    ak, bk = case['era']['ak'], case['era']['bk']
    lvl1 = np.arange(1, len(ak) + 1)
    pa_hl_pgw, pa_pgw = F.hybrid_pressure(ak, bk, out['PS'])
    # QV written by the path == rh_to_q(hur_pgw, pa(final ps), ta_pgw)   (step_03:262-266,370)
    q2 = F.relative_to_specific_humidity(out['_hur_pgw'], pa_pgw, out['T'])
    np.testing.assert_allclose(q2.numpy(), out['QV'].numpy(), rtol=1e-12, atol=1e-18)
    phi_pgw = F.integ_geopot(pa_hl_pgw, era['FIS'], out['T'], out['QV'], lvl1, 30000.0).numpy()
    pa_hl_era, _ = F.hybrid_pressure(ak, bk, era['PS'])
    phi_era = F.integ_geopot(pa_hl_era, era['FIS'], era['T'], era['QV'], lvl1, 30000.0).numpy()
    kref = int(np.nonzero(case['plev'] == 30000.0)[0][0])
    dzg = O.load_delta_values(case['deltas']['zg'][:, kref], case['delta_times'], case['target_dt'])
    err = (phi_pgw - phi_era) - dzg * O.CON_G
    assert abs(np.abs(err).max() - info['max_err'][-1]) < 1e-7
    # early exit above p_ref gives the same phi as the full-column scan
    phi_ee = F.integ_geopot(pa_hl_pgw, era['FIS'], out['T'], out['QV'], lvl1, 30000.0, full_column=False).numpy()
    np.testing.assert_array_equal(phi_ee, phi_pgw)


def test_full_size_analytic_and_linearity(full_case):
    """Analytic / algebraic properties at 1440x721xL137: isothermal dry column is exact;
    interp_logp_4d reproduces a profile linear in ln p; the delta interpolation is linear in the
    delta values."""
    from pgw4era5_amd import functions as F
    ctx, case, era, out, info = full_case
    ak, bk = case['era']['ak'], case['era']['bk']
    pa_hl, pa = F.hybrid_pressure(ak, bk, era['PS'])
    shp = pa.shape
    T = ctx.to_device(np.full(shp, 250.0), np.float64)
    q = ctx.zeros(shp, np.float64)
    phi = F.integ_geopot(pa_hl, era['FIS'], T, q, np.arange(1, shp[1] + 2), 30000.0).numpy()
    np.testing.assert_allclose(phi, case['era']['FIS'] + O.CON_RD * 250.0 * np.log(case['era']['PS'] / 30000.0), rtol=1e-11)
    T.free(); q.free()
    pa_h = pa.numpy()
    prof = 3.0 + 2.0 * np.log(pa_h[:, ::7])                 # 20 source levels of the same column
    got = F.interp_logp_4d(prof, pa_h[:, ::7], pa_h[:, 3:130], 'off')
    np.testing.assert_allclose(got, 3.0 + 2.0 * np.log(pa_h[:, 3:130]), rtol=1e-12)
    del prof, got
    d1 = case['deltas']['ua'][6:7]; d2 = case['deltas']['va'][6:7]
    a = F.vert_interp_delta(d1, pa, None, None, True, plev=case['plev']).numpy()
    b = F.vert_interp_delta(d2, pa, None, None, True, plev=case['plev']).numpy()
    c = F.vert_interp_delta(2.0 * d1 - 0.5 * d2, pa, None, None, True, plev=case['plev']).numpy()
    np.testing.assert_allclose(c, 2.0 * a - 0.5 * b, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ p_ref_inp = None (SURVEY 8 f, rank 2)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_local_p_ref_mode_vs_oracle(dtype):
    """settings.p_ref_inp = None: reference pressure chosen per column and per pass
    (reference step_03_apply_to_era.py:219-253, functions.py:583-598)."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    c = _case(9, 14, 30, seed=21, dtype=dtype)
    got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref='local',
                                 ref_dtype=False)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    era = {k: (f64(v) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in c['era'].items()}
    d = {k: f64(v) for k, v in c['deltas'].items()}
    akm, bkm = O.full_level_coeffs(era['ak'], era['bk'])
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'], akm, bkm)
    ld = lambda k: O.load_delta_values(d[k], c['delta_times'], c['target_dt'])
    ta = era['T'] + O.vert_interp_delta(ld('ta'), c['plev'], pa, ld('tas'), ld('ps_hist'), True)
    hur = O.specific_to_relative_humidity(era['QV'], pa, era['T']) + \
        O.vert_interp_delta(ld('hur'), c['plev'], pa, ld('hurs'), ld('ps_hist'), True)
    want = O.adjust_ps_loop_local_pref(era['ak'], era['bk'], akm, bkm, era['PS'], era['FIS'], era['T'], era['QV'],
                                       ta, hur, ld('zg'), c['plev'])
    assert len(np.unique(want['p_ref'])) > 1            # mountains pick a higher reference level than sea points
    assert got['n_iter'] == want['n_iter']
    tol = 1e-9 if dtype == np.float64 else 1e-6
    np.testing.assert_allclose(got['PS'], want['ps_pgw'], rtol=tol)
    np.testing.assert_allclose(got['QV'], want['hus_pgw'], rtol=tol if dtype == np.float64 else 3e-6, atol=1e-18)
    np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=1e-6 if dtype == np.float64 else 1e-5, atol=1e-7)
    # one launch per pass (k_local_p_ref + two scans, the first form) against the multi-pass kernel's LOCAL variant, and first
    # launches shorter than the file needs (continuation launches resume the per-column level memory): the same bits
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    for opts in (dict(multipass=0), dict(loop_guess=1), dict(loop_guess=3)):
        old = {k: ctx.set_option(k, v) for k, v in opts.items()}
        try:
            alt = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref='local',
                                         ref_dtype=False)
        finally:
            for k, v in old.items():
                if k != 'loop_guess':
                    ctx.set_option(k, v)
        assert alt['n_iter'] == got['n_iter'] and alt['max_err'] == got['max_err'], opts
        for k in ('PS', 'QV', 'T'):
            np.testing.assert_array_equal(alt[k], got[k], err_msg=str(opts) + k)
    if dtype == np.float32:
        # reference-dtype mode with the local reference level (float32 delta_ps / ps_pgw / phi): same pass count here,
        # PS within the float32 noise floor of the fast mode
        ref = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref='local',
                                     ref_dtype=True)
        assert ref['T'].dtype == np.float64 and ref['PS'].dtype == np.float32
        assert ref['n_iter'] == got['n_iter']
        np.testing.assert_allclose(ref['PS'], got['PS'], rtol=1.5e-6)


def _mixed_axes_case(dtype, seed=31):
    """A small file whose delta files have different time axes: ta, hur, va, tas, hurs, ps_hist monthly; ua on 24
    half-month stamps (a member of the quad group on another axis); zg on 6 stamps; tos / siconc monthly but on other
    days of the month; ts seasonal; the 3-D model-level variables also daily-ish in a second variant."""
    from pgw4era5_amd import synthetic
    c = synthetic.make_case(7, 9, 18, seed=seed, dtype=dtype)
    day = np.timedelta64(1, 'D')
    y0 = np.datetime64('1995-01-01T00:00:00')
    stamps = dict(ua=y0 + np.arange(24) * 15 * day + 7 * day,
                  zg=y0 + np.arange(6) * 61 * day + 30 * day,
                  tos=y0 + np.arange(12) * 30 * day + 3 * day + np.timedelta64(6, 'h'),
                  siconc=y0 + np.arange(12) * 30 * day + 3 * day + np.timedelta64(6, 'h'),
                  ts=y0 + np.arange(4) * 91 * day + 45 * day)
    deltas, times = synthetic.resample_deltas(c, stamps, seed=seed)
    return c, deltas, times


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_per_variable_delta_time_axes_vs_oracle(dtype):
    """The reference loads every delta file on its own (load_delta, functions.py:195-303): each variable is bracketed and
    interpolated on ITS time axis.  Instants: inside the year, before every first record (wrap to the previous year), after
    every last one, and exactly on a tos / siconc record (no interpolation for those two, functions.py:282-283).  float64
    file against the float64 oracle, float32 file (reference-dtype mode) against the reference-dtype oracle; the record
    window (resident=False) gives the bits of the resident set."""
    import datetime as dt
    from pgw4era5_amd import step_03_apply_to_era as s3
    c, deltas, times = _mixed_axes_case(dtype)
    ora = O if dtype == np.float64 else R
    on_tos_record = times['tos'][4].astype(dt.datetime).replace(year=2006)
    for target in (dt.datetime(2006, 8, 2, 3), dt.datetime(2006, 1, 1, 0), dt.datetime(2006, 12, 31, 21), on_tos_record):
        got = s3.pgw_for_era5_arrays(c['era'], deltas, times, c['plev'], target, True)
        want = ora.pgw_for_era5_arrays(c['era'], deltas, times, c['plev'], target, True)
        assert got['n_iter'] == want['n_iter'], target
        if dtype == np.float64:
            for k in ['PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE']:
                np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12, equal_nan=True, err_msg='%s %s' % (k, target))
        else:
            for k in ['PS', 'T_SKIN', 'T_SO', 'FR_SEA_ICE']:
                np.testing.assert_allclose(got[k], want[k], rtol=2.5e-7, atol=1e-7, equal_nan=True, err_msg='%s %s' % (k, target))
            np.testing.assert_allclose(got['T'], want['T'], rtol=1e-9, err_msg=str(target))
            np.testing.assert_allclose(got['V'], want['V'], rtol=1e-9, atol=1e-9, err_msg=str(target))
            # ua sits on another axis than ta: it is interpolated in time before the quad kernel and held as ONE float32
            # field there (the fused path keeps the float64 value): one float32 rounding of a delta of a few m/s
            np.testing.assert_allclose(got['U'], want['U'], rtol=0, atol=4e-7 * np.abs(deltas['ua']).max() + 1e-9, err_msg=str(target))
        win = s3.pgw_for_era5_arrays(c['era'], deltas, times, c['plev'], target, True, resident=False)
        assert win['n_iter'] == got['n_iter']
        for k in ['PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE']:
            np.testing.assert_array_equal(win[k], got[k], err_msg='window %s' % k)
    # the same time axis handed over per variable is the one-axis call, bit for bit
    one = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    per = s3.pgw_for_era5_arrays(c['era'], c['deltas'], {k: c['delta_times'] for k in c['deltas']}, c['plev'], c['target_dt'], True)
    for k in ['PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE']:
        np.testing.assert_array_equal(one[k], per[k], err_msg=k)


def test_delta_record_window_keeps_few_records_on_the_device():
    """DeltaSet with resident=False: at most WINDOW records of a variable live on the device, a record is uploaded once
    while consecutive instants need it, and walking through the year (and across its end) returns the resident set's
    records bit for bit."""
    import datetime as dt
    from pgw4era5_amd import step_03_apply_to_era as s3, synthetic
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    c = synthetic.make_case(4, 6, 10, seed=5)
    day = np.timedelta64(1, 'D')
    daily = np.datetime64('1996-01-01T12:00:00') + np.arange(366) * day            # a leap year: Feb 29 is dropped
    deltas, times = synthetic.resample_deltas(c, {k: daily for k in ('ta', 'hur', 'ua', 'va', 'zg', 'tas', 'hurs')}, seed=2)
    reads = []

    class Provider:                                   # the interface of ncio.RecordReader over an in-memory array
        def __init__(self, name, arr):
            self.name, self.arr, self.nrec, self.rec_shape = name, arr, arr.shape[0], arr.shape[1:]

        def read_record(self, r):
            reads.append((self.name, r))
            return self.arr[r]
    win = s3.DeltaSet(ctx, {k: Provider(k, v) for k, v in deltas.items()}, None, c['plev'], np.float64, times_by_var=times, resident=False)
    res = s3.DeltaSet(ctx, deltas, None, c['plev'], np.float64, times_by_var=times, resident=True)
    assert not win.resident and res.resident and not win.dev
    t = dt.datetime(2007, 2, 27, 0)
    n_ts_reads = len([x for x in reads if x[0] == 'ts'])                            # ts was walked once for its annual mean
    assert n_ts_reads == 12
    del reads[:]
    for step in range(40):                                                          # 3-hourly over Feb 28 -> Mar 3
        for var in ('ta', 'tas', 'tos'):
            b0, a0, x0, n0 = win.pair(var, t, None)
            b1, a1, x1, n1 = res.pair(var, t, None)
            assert (x0, n0) == (x1, n1)
            np.testing.assert_array_equal(b0.numpy(), b1.numpy())
            np.testing.assert_array_equal(a0.numpy(), a1.numpy())
        assert all(len(cache) <= s3.DeltaSet.WINDOW for cache in win._cache.values())
        t += dt.timedelta(hours=3)
    ta_reads = [r for v, r in reads if v == 'ta']
    assert len(ta_reads) == len(set(ta_reads)) <= 7                                 # five days: each record uploaded once
    assert 59 not in ta_reads                                                       # record 59 = Feb 29, never needed
    b, a, x_hi, x_new = win.pair('ta', dt.datetime(2007, 12, 31, 18), None)         # after the last record: wraps to the first
    np.testing.assert_array_equal(a.numpy(), deltas['ta'][0])
    np.testing.assert_array_equal(b.numpy(), deltas['ta'][365])
    assert x_hi == 86400e9 and x_new == 6 * 3600e9
    win.free(); res.free()


def test_local_p_ref_no_candidate_error():
    from pgw4era5_amd import step_03_apply_to_era as s3
    c = _case(4, 5, 12, seed=22)
    keep = c['plev'] >= 85000.0                      # deltas that only reach 850 hPa
    d = {k: (v[:, keep] if v.ndim == 4 else v.copy()) for k, v in c['deltas'].items()}
    # every column above the delta top (ps_hist > 850 hPa, else replace_delta_sfc raises first), but one
    # column with 0.95 * ps below 850 hPa: no reference level for it
    c['era']['PS'][:] = np.maximum(c['era']['PS'], 95000.0)
    d['ps_hist'][:] = np.maximum(d['ps_hist'], 95000.0)
    c['era']['PS'][0, 0, 0] = 88000.0
    d['ps_hist'][:, 0, 0] = 88000.0
    with pytest.raises(ValueError) as e:
        s3.pgw_for_era5_arrays(c['era'], d, c['delta_times'], c['plev'][keep], c['target_dt'], True, p_ref='local')
    assert 'No reference pressure level' in str(e.value)


# ------------------------------------------------------------------ i_reinterp = 1 (SURVEY 8 f, rank 3)
@pytest.mark.parametrize('p_ref', ['fixed', 'local'])
@pytest.mark.parametrize('mode', ['f64', 'f32_reference', 'f32_fast'])
def test_reinterp_mode_vs_oracle(mode, p_ref):
    """settings.i_reinterp = 1: ERA fields and deltas re-interpolated onto the updated model levels in every pass, ua / va
    after convergence (reference step_03_apply_to_era.py:202-216, 330-343) - with the fixed reference level and with
    p_ref_inp = None (:219-253; independent switches in the reference), on a float64 file against the float64 oracle, on a
    float32 file in reference-dtype mode against the reference-dtype oracle (float64 T / QV / U / V out: interp_logp_4d
    returns float64, functions.py:472-477; float32 value differences of the float32 ERA temperature, :575-578; float32
    delta_ps / ps_pgw / phi_hl) and in fast mode (float64 arithmetic, float32 outputs) against the float64 oracle."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    dtype = np.float64 if mode == 'f64' else np.float32
    c = _case(8, 10, 24, seed=31, dtype=dtype)
    pr = None if p_ref == 'local' else 30000.0
    args = (c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    got = s3.pgw_for_era5_arrays(*args, i_reinterp=True, p_ref='local' if p_ref == 'local' else None,
                                 ref_dtype=None if mode == 'f64' else (mode == 'f32_reference'))
    if mode == 'f32_reference':
        want = R.pgw_for_era5_arrays_reinterp(*args, p_ref=pr)
        assert got['T'].dtype == np.float64 and got['U'].dtype == np.float64 and got['QV'].dtype == np.float64
        assert got['PS'].dtype == np.float32
        tol = dict(PS=2.5e-7, T=1e-9, QV=6e-7)
    else:
        want = O.pgw_for_era5_arrays_reinterp(c['era'], {k: np.asarray(v, dtype=np.float64) for k, v in c['deltas'].items()},
                                              *args[2:], p_ref=pr)
        tol = dict(PS=1e-9, T=1e-9, QV=1e-9) if mode == 'f64' else dict(PS=2e-6, T=2e-6, QV=5e-6)
    assert got['n_iter'] == want['n_iter']
    np.testing.assert_allclose(np.asarray(got['max_err']), np.asarray(want['max_err']), rtol=1e-6 if mode == 'f64' else 0.2, atol=1e-7)
    np.testing.assert_allclose(got['PS'], want['PS'], rtol=tol['PS'], err_msg='PS')
    if mode == 'f32_reference':
        # ps_pgw may sit one float32 ulp beside the oracle's (the device logarithm against numpy's); the
        # re-interpolated fields carry that 6e-8 relative pressure shift times their vertical gradient: white noise in the
        # synthetic winds (sigma 10 m/s per level), a lapse rate in T
        np.testing.assert_allclose(got['T'], want['T'], rtol=6e-8, err_msg='T')
        for k in ('U', 'V'):
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=2e-5, err_msg=k)
    else:
        for k in ['T', 'U', 'V']:
            np.testing.assert_allclose(got[k], want[k], rtol=tol['T'], atol=1e-5 if mode != 'f64' else 1e-9, err_msg=k)
    scale = np.nanmax(np.abs(want['QV']), axis=(2, 3), keepdims=True)
    assert np.nanmax(np.abs(got['QV'] - want['QV']) / scale) < tol['QV']
    if p_ref == 'local':
        assert len(np.unique(want['p_ref'])) > 1            # mountains pick a higher reference level than sea points
    # differs from the default mode (deltas interpolated once on the ERA levels)
    base = s3.pgw_for_era5_arrays(*args, p_ref='local' if p_ref == 'local' else None,
                                  ref_dtype=None if mode == 'f64' else (mode == 'f32_reference'))
    assert np.abs(base['T'].astype(np.float64) - got['T']).max() > 1e-6


@pytest.mark.parametrize('p_ref', [None, 'local'])
def test_reinterp_reference_dtype_mode_with_64_bit_offsets_is_bit_identical(p_ref):
    """The 64-bit byte-offset instantiations of k_reinterp_pair's mixed-type forms (float32 ERA field, float64 RELHUM and
    outputs: the second field's and the outputs' offsets are the first field's scaled by the element-size ratio) - the
    path arrays of 4 GiB and more take - give the bits of the 32-bit ones."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    c = _case(6, 9, 21, seed=35, dtype=np.float32)
    args = (c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    a = s3.pgw_for_era5_arrays(*args, i_reinterp=True, p_ref=p_ref, ref_dtype=True)
    old = ctx.set_option('force_off64', 1)
    try:
        b = s3.pgw_for_era5_arrays(*args, i_reinterp=True, p_ref=p_ref, ref_dtype=True)
    finally:
        ctx.set_option('force_off64', old)
    assert a['n_iter'] == b['n_iter'] and a['max_err'] == b['max_err']
    for k in ('PS', 'T', 'QV', 'U', 'V'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reinterp_one_call_path_is_the_host_composed_path_bit_for_bit(dtype):
    """pgw_step03_file with i_reinterp (one C call per file) against the same path composed on the host from the
    function-level entries (pgw_reinterp_pass per pass, pgw_reinterp_pair for ua / va, the humidity entries): fixed p_ref,
    float64 arithmetic on the storage type - the same bits, pass count and max|err| history included."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    c = _case(7, 11, 22, seed=33, dtype=dtype)
    ds = s3.DeltaSet(ctx, c['deltas'], c['delta_times'], c['plev'], dtype)
    e = s3._upload_era(ctx, c['era'], dtype)
    coeffs = dict(ak=c['era']['ak'], bk=c['era']['bk'], soil1=c['era']['soil1'])
    o1, i1 = s3.process_file_device_reinterp(ctx, e, coeffs, ds, c['target_dt'], True, ref_dtype=False)
    o2, i2 = s3.process_file_device_reinterp_composed(ctx, e, coeffs, ds, c['target_dt'], True)
    assert i1['n_iter'] == i2['n_iter'] and i1['max_err'] == i2['max_err']
    for k in ('PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE'):
        if k == 'QV' and dtype == np.float32:
            # float32 storage, fast mode: the one-call path takes QV from the stored vapour pressure e (one float32 rounding of
            # e), the composed path from the stored hur_pgw (one float32 rounding of hur): two float32 ulp apart at most
            np.testing.assert_allclose(o1[k].numpy(), o2[k].numpy(), rtol=2.5e-7, atol=1e-12, err_msg=k)
        else:
            np.testing.assert_array_equal(o1[k].numpy(), o2[k].numpy(), err_msg=k)
    ds.free()


@pytest.mark.parametrize('with_sfc', [True, False])
def test_reinterp_field_kernel_vs_oracle_composition(with_sfc):
    """pgw_reinterp_field alone: interp_logp_4d(era, pa_era, pa_pgw, 'constant') + vert_interp_delta(delta, pa_pgw) of the
    oracle, with surface pressures far apart (+-8 %: the re-interpolation extrapolates at both ends of the column and the
    window over the ERA column moves by several levels), an exact record and a time-interpolated one."""
    import ctypes as C
    from pgw4era5_amd.device import default_context, dtype_tag
    ctx = default_context()
    c = _case(7, 9, 23, seed=33)
    era, d = c['era'], c['deltas']
    ctx.set_levels(era['ak'], era['bk'])
    rng = np.random.default_rng(5)
    ps_era = era['PS']
    ps_pgw = ps_era * (1 + 0.08 * (2 * rng.random(ps_era.shape) - 1))
    akm, bkm = O.full_level_coeffs(era['ak'], era['bk'])
    _, pa_era = O.hybrid_pressure(era['ak'], era['bk'], ps_era, akm, bkm)
    _, pa_pgw = O.hybrid_pressure(era['ak'], era['bk'], ps_pgw, akm, bkm)
    nt, N, nlat, nlon = era['T'].shape
    ncol = nlat * nlon
    plev = np.ascontiguousarray(c['plev'], dtype=np.float64)
    dp = C.POINTER(C.c_double)
    for rb, ra, x_hi, x_new in ((3, 3, 0.0, 0.0), (3, 4, 31.0, 11.5)):
        if x_hi == 0.0:
            delta, dsfc, psh = d['ta'][rb:rb + 1], d['tas'][rb:rb + 1], d['ps_hist'][rb:rb + 1]
        else:
            lerp = lambda v: (v[ra:ra + 1] - v[rb:rb + 1]) / x_hi * x_new + v[rb:rb + 1]
            delta, dsfc, psh = lerp(d['ta']), lerp(d['tas']), lerp(d['ps_hist'])
        want = O.interp_logp_4d(era['T'], pa_era, pa_pgw, extrapolate='constant') + \
            O.vert_interp_delta(delta, c['plev'], pa_pgw, dsfc if with_sfc else None, psh if with_sfc else None,
                                ignore_top_pressure_error=True)
        dev = {k: ctx.to_device(np.ascontiguousarray(v)) for k, v in
               dict(f=era['T'], pe=ps_era, pp=ps_pgw, db=d['ta'][rb], da=d['ta'][ra], sb=d['tas'][rb], sa=d['tas'][ra],
                    hb=d['ps_hist'][rb], ha=d['ps_hist'][ra]).items()}
        out = ctx.empty(era['T'].shape, np.float64)
        sfc = (dev['sb'].ptr, dev['sa'].ptr, dev['hb'].ptr, dev['ha'].ptr) if with_sfc else (None, None, None, None)
        ctx._check(ctx.lib.pgw_reinterp_field(ctx.handle, dtype_tag(np.dtype('float64')), nt, len(plev), ncol, plev.ctypes.data_as(dp),
                                              dev['db'].ptr, dev['da'].ptr, x_hi, x_new, *sfc, dev['f'].ptr, dev['pe'].ptr,
                                              dev['pp'].ptr, 1, out.ptr))
        np.testing.assert_allclose(out.numpy(), want, rtol=1e-10, atol=1e-12)
    # identical surface pressures: the re-interpolated ERA field is the field itself (exact hits, functions.py:540-543)
    ctx._check(ctx.lib.pgw_reinterp_field(ctx.handle, dtype_tag(np.dtype('float64')), nt, len(plev), ncol, plev.ctypes.data_as(dp),
                                          dev['db'].ptr, dev['da'].ptr, 0.0, 0.0, *sfc, dev['f'].ptr, dev['pe'].ptr, dev['pe'].ptr,
                                          1, out.ptr))
    same = O.vert_interp_delta(d['ta'][rb:rb + 1], c['plev'], pa_era, d['tas'][rb:rb + 1] if with_sfc else None,
                               d['ps_hist'][rb:rb + 1] if with_sfc else None, ignore_top_pressure_error=True)
    np.testing.assert_allclose(out.numpy() - era['T'], same, rtol=0, atol=1e-10)
    # the model-top check is the one of vert_interp_delta (functions.py:417-425)
    with pytest.raises(ValueError) as e:
        ctx._check(ctx.lib.pgw_reinterp_field(ctx.handle, dtype_tag(np.dtype('float64')), nt, len(plev), ncol, plev.ctypes.data_as(dp),
                                              dev['db'].ptr, dev['da'].ptr, 0.0, 0.0, *sfc, dev['f'].ptr, dev['pe'].ptr,
                                              dev['pp'].ptr, 0, out.ptr))
    assert 'ERA5 top pressure is lower than climate delta top pressure' in str(e.value)


@pytest.mark.parametrize('off64', [0, 1])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reinterp_pair_is_two_reinterp_fields_bit_for_bit(dtype, off64, request):
    """pgw_reinterp_pair (ta + hur with the surface insertion, ua + va without) == two pgw_reinterp_field calls, bit for bit:
    surface pressures +-8 % apart, a time-interpolated instant and an exact record, a column with a NaN surface pressure
    (both scans restart) and ps_hist above / inside / at the edge of the delta levels."""
    import ctypes as C
    from pgw4era5_amd.device import default_context, dtype_tag
    ctx = default_context()
    ctx.set_option('force_off64', off64)            # 1: the 64-bit byte-offset instantiation (arrays of 4 GiB and more)
    request.addfinalizer(lambda: ctx.set_option('force_off64', 0))
    c = _case(7, 9, 23, seed=35, dtype=dtype)
    era, d = c['era'], c['deltas']
    ctx.set_levels(era['ak'], era['bk'])
    rng = np.random.default_rng(6)
    ps_era = era['PS'].copy()
    ps_pgw = (ps_era * (1 + 0.08 * (2 * rng.random(ps_era.shape) - 1))).astype(dtype)
    ps_pgw[0, 2, 3] = np.nan
    psh = d['ps_hist'].copy()
    psh[:, 0, 0] = 103000.0                 # above every delta level: the last level moves
    psh[:, 0, 1] = 70010.0                  # inside
    nt, N, nlat, nlon = era['T'].shape
    ncol = nlat * nlon
    plev = np.ascontiguousarray(c['plev'], dtype=np.float64)
    dp = C.POINTER(C.c_double)
    tag = dtype_tag(np.dtype(dtype))
    up = lambda v: ctx.to_device(np.ascontiguousarray(v, dtype=dtype))
    pe, pp = up(ps_era), up(ps_pgw)
    arr = lambda a, b: (C.c_void_p * 2)(a.ptr, b.ptr)
    for (v0, v1, f0, f1, with_sfc) in (('ta', 'hur', era['T'], era['QV'] * 1e4, True), ('ua', 'va', era['U'], era['V'], False)):
        for rb, ra, x_hi, x_new in ((3, 3, 0.0, 0.0), (3, 4, 31.0, 11.5)):
            D = {k: up(v) for k, v in dict(f0=f0, f1=f1, b0=d[v0][rb], a0=d[v0][ra], b1=d[v1][rb], a1=d[v1][ra]).items()}
            if with_sfc:
                D.update({k: up(v) for k, v in dict(s0b=d[v0 + 's'][rb], s0a=d[v0 + 's'][ra], s1b=d[v1 + 's'][rb],
                                                    s1a=d[v1 + 's'][ra], hb=psh[rb], ha=psh[ra]).items()})
            single = []
            for i in (0, 1):
                out = ctx.empty(era['T'].shape, dtype)
                sfc = (D['s%db' % i].ptr, D['s%da' % i].ptr, D['hb'].ptr, D['ha'].ptr) if with_sfc else (None,) * 4
                ctx._check(ctx.lib.pgw_reinterp_field(ctx.handle, tag, nt, len(plev), ncol, plev.ctypes.data_as(dp), D['b%d' % i].ptr,
                                                      D['a%d' % i].ptr, x_hi, x_new, *sfc, D['f%d' % i].ptr, pe.ptr, pp.ptr, 1, out.ptr))
                single.append(out.numpy())
            o0, o1 = ctx.empty(era['T'].shape, dtype), ctx.empty(era['T'].shape, dtype)
            sfc = (arr(D['s0b'], D['s1b']), arr(D['s0a'], D['s1a']), D['hb'].ptr, D['ha'].ptr) if with_sfc else (None,) * 4
            ctx._check(ctx.lib.pgw_reinterp_pair(ctx.handle, tag, nt, len(plev), ncol, plev.ctypes.data_as(dp), arr(D['b0'], D['b1']),
                                                 arr(D['a0'], D['a1']), x_hi, x_new, *sfc, arr(D['f0'], D['f1']), pe.ptr, pp.ptr, 1,
                                                 arr(o0, o1)))
            np.testing.assert_array_equal(o0.numpy(), single[0])
            np.testing.assert_array_equal(o1.numpy(), single[1])
    # the model-top check of vert_interp_delta (functions.py:417-425); a NaN in the target pressures makes numpy's
    # comparison False (no error), so this one runs on the NaN-free surface pressures
    ctx._check(ctx.lib.pgw_reinterp_pair(ctx.handle, tag, nt, len(plev), ncol, plev.ctypes.data_as(dp), arr(D['b0'], D['b1']),
                                         arr(D['a0'], D['a1']), 0.0, 0.0, None, None, None, None, arr(D['f0'], D['f1']), pe.ptr,
                                         pp.ptr, 0, arr(o0, o1)))
    with pytest.raises(ValueError) as e:
        ctx._check(ctx.lib.pgw_reinterp_pair(ctx.handle, tag, nt, len(plev), ncol, plev.ctypes.data_as(dp), arr(D['b0'], D['b1']),
                                             arr(D['a0'], D['a1']), 0.0, 0.0, None, None, None, None, arr(D['f0'], D['f1']), pe.ptr,
                                             pe.ptr, 0, arr(o0, o1)))
    assert 'ERA5 top pressure is lower than climate delta top pressure' in str(e.value)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reinterp_pass_is_its_three_steps_bit_for_bit(dtype):
    """pgw_reinterp_pass (one call per loop pass of i_reinterp = 1) == pgw_update_ps + pgw_reinterp_pair(ta, hur) +
    pgw_adjust_ps_step(apply_adj = 0): ps_pgw, ta_pgw, hur_pgw, delta_ps, adj_ps and max |err| over two passes."""
    import ctypes as C
    from pgw4era5_amd.device import default_context, dtype_tag
    from pgw4era5_amd import step_03_apply_to_era as s3
    ctx = default_context()
    c = _case(7, 9, 23, seed=37, dtype=dtype)
    era, d = c['era'], c['deltas']
    ctx.set_levels(era['ak'], era['bk'])
    nt, N, nlat, nlon = era['T'].shape
    ncol, tag = nlat * nlon, dtype_tag(np.dtype(dtype))
    plev = np.ascontiguousarray(c['plev'], dtype=np.float64)
    dp = C.POINTER(C.c_double)
    up = lambda v, t=dtype: ctx.to_device(np.ascontiguousarray(v, dtype=t))
    rb, ra, x_hi, x_new = 3, 4, 31.0, 11.5
    D = {k: up(v) for k, v in dict(T=era['T'], RH=O.specific_to_relative_humidity(era['QV'].astype(np.float64),
                                                                                   O.hybrid_pressure(era['ak'], era['bk'], era['PS'].astype(np.float64))[1],
                                                                                   era['T'].astype(np.float64)),
                                   PS=era['PS'], FIS=era['FIS'], tb=d['ta'][rb], ta=d['ta'][ra], hb=d['hur'][rb], ha=d['hur'][ra],
                                   tsb=d['tas'][rb], tsa=d['tas'][ra], hsb=d['hurs'][rb], hsa=d['hurs'][ra],
                                   pb=d['ps_hist'][rb], pa=d['ps_hist'][ra]).items()}
    rng = np.random.default_rng(3)
    phi_era = up(rng.normal(5.0e4, 10.0, era['PS'].shape), np.float64)
    dphi = up(rng.normal(300.0, 30.0, era['PS'].shape), np.float64)
    arr = lambda a, b: (C.c_void_p * 2)(a.ptr, b.ptr)
    res = []
    for fused in (False, True):
        dps, adj = up(np.zeros(era['PS'].shape), np.float64), up(rng.normal(0.0, 0.0, era['PS'].shape) + 25.0, np.float64)
        ps, ta, hur = ctx.empty(era['PS'].shape, dtype), ctx.empty(era['T'].shape, dtype), ctx.empty(era['T'].shape, dtype)
        errs = []
        for _ in range(2):
            me = C.c_double()
            if fused:
                ctx._check(ctx.lib.pgw_reinterp_pass(ctx.handle, tag, nt, len(plev), ncol, plev.ctypes.data_as(dp), arr(D['tb'], D['hb']),
                                                     arr(D['ta'], D['ha']), x_hi, x_new, arr(D['tsb'], D['hsb']), arr(D['tsa'], D['hsa']),
                                                     D['pb'].ptr, D['pa'].ptr, D['T'].ptr, D['RH'].ptr, D['PS'].ptr, D['FIS'].ptr,
                                                     phi_era.ptr, dphi.ptr, dps.ptr, adj.ptr, 30000.0, 0.95, 1, ps.ptr, ta.ptr, hur.ptr,
                                                     C.byref(me)))
            else:
                ctx._check(ctx.lib.pgw_update_ps(ctx.handle, tag, nt * ncol, D['PS'].ptr, dps.ptr, adj.ptr, ps.ptr))
                ctx._check(ctx.lib.pgw_reinterp_pair(ctx.handle, tag, nt, len(plev), ncol, plev.ctypes.data_as(dp), arr(D['tb'], D['hb']),
                                                     arr(D['ta'], D['ha']), x_hi, x_new, arr(D['tsb'], D['hsb']), arr(D['tsa'], D['hsa']),
                                                     D['pb'].ptr, D['pa'].ptr, arr(D['T'], D['RH']), D['PS'].ptr, ps.ptr, 1, arr(ta, hur)))
                ctx._check(ctx.lib.pgw_adjust_ps_step(ctx.handle, tag, nt, ncol, ta.ptr, hur.ptr, D['PS'].ptr, D['FIS'].ptr, phi_era.ptr,
                                                      dphi.ptr, dps.ptr, adj.ptr, 30000.0, None, 0.95, 0, C.byref(me)))
            errs.append(me.value)
        res.append(dict(ps=ps.numpy(), ta=ta.numpy(), hur=hur.numpy(), dps=dps.numpy(), adj=adj.numpy(), errs=errs))
    a, b = res
    assert a['errs'] == b['errs'] and np.isfinite(a['errs']).all() and a['errs'][0] != a['errs'][1]
    for k in ('ps', 'ta', 'hur', 'dps', 'adj'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_reference_dtype_mode_with_64_bit_offsets_is_bit_identical():
    """float32 file, reference-dtype mode, through the 64-bit byte-offset instantiation of k_delta_quad."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    c = _case(8, 12, 27, seed=82, dtype=np.float32)
    args = (c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    a = s3.pgw_for_era5_arrays(*args)
    old = ctx.set_option('force_off64', 1)
    try:
        b = s3.pgw_for_era5_arrays(*args)
    finally:
        ctx.set_option('force_off64', old)
    assert a['n_iter'] == b['n_iter'] and a['max_err'] == b['max_err']
    for k in ['PS', 'T', 'QV', 'U', 'V']:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_file_path_on_arrays_of_more_than_4_GiB():
    """A 0.125 deg-sized file (4.17 M columns, L137, float64: 4.57 GB per 4-D field) takes the 64-bit byte-offset
    instantiations and 64-bit index arithmetic for real.  Size-independent property: 16 copies of a 181 x 1440 file along
    latitude give 16 copies of that file's result, bit for bit, with the same pass count and max|err| history
    (tools/big_grid_check.py).  Needs ~90 GB of HBM and ~80 GB of host memory (skipped on a smaller machine)."""
    import importlib.util
    import psutil
    from pgw4era5_amd.device import default_context
    free, _ = default_context().mem_info()
    if free < 120e9 or psutil.virtual_memory().available < 120e9:
        pytest.skip('needs 120 GB of free HBM and of host memory')
    spec = importlib.util.spec_from_file_location('big_grid_check', os.path.join(ROOT, 'tools', 'big_grid_check.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main() == 0


def test_randomised_parity_sweep():
    """tools/fuzz_parity.py: 400 small random files - grids down to one column, 8..44 levels, float32 (reference mode) and
    float64, plev subsets, time stamps at records / across the year wrap, ps_hist above the delta levels, the fixed and the
    local reference level, i_reinterp - HIP path against the oracles with this file's tolerances; no disagreement."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location('fuzz_parity', os.path.join(ROOT, 'tools', 'fuzz_parity.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = sys.argv
    sys.argv = ['fuzz_parity.py', '--cases', '400', '--seed', '2']
    try:
        assert mod.main() == 0
    finally:
        sys.argv = argv


def test_randomised_function_level_sweep():
    """tools/fuzz_functions.py: 600 random calls of the function-level entries (interp_logp_4d in its four modes against the
    serial C column loops, vert_interp_delta, integ_geopot, humidity, regrid_field, smooth_annual_cycle) incl. their error
    cases: values within the tolerances of this file, the same exception on both sides."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location('fuzz_functions', os.path.join(ROOT, 'tools', 'fuzz_functions.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = sys.argv
    sys.argv = ['fuzz_functions.py', '--cases', '600', '--seed', '3']
    try:
        assert mod.main() == 0
    finally:
        sys.argv = argv


def test_loop_non_convergence_raises_the_reference_error(monkeypatch):
    """it > max_n_iter raises even if that pass converged (step_03:313-319)."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    import pgw4era5_amd.settings as S
    c = _case(9, 16, 30, seed=41)
    a = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    monkeypatch.setattr(S, 'max_n_iter', a['n_iter'])
    with pytest.raises(ValueError) as e:
        s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    assert 'did not converge' in str(e.value)
    monkeypatch.setattr(S, 'max_n_iter', a['n_iter'] + 1)
    b = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    assert b['n_iter'] == a['n_iter']


# ------------------------------------------------------------------ reference-dtype mode (float32 ERA5 files)
def _scaled_qv_diff(a, b):
    """max |a - b| relative to each level's largest value (hur_pgw crosses zero in the dry stratosphere, where a
    pointwise relative difference says nothing)."""
    scale = np.nanmax(np.abs(b), axis=(2, 3), keepdims=True)
    return np.nanmax(np.abs(a - b) / scale)


@pytest.mark.parametrize('delta_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape,seed', [((10, 10, 20), 0), ((24, 36, 60), 1), ((7, 13, 21), 2), ((3, 5, 137), 3)])
def test_reference_dtype_mode_vs_refdtype_oracle(shape, seed, delta_dtype):
    """float32 ERA5 file in the default mode (settings.f32_file_mode = 'reference', pgw_file_args.ref_dtype = 1) against
    oracle/pgw_oracle_refdtype.py, which follows numpy's promotion through the reference's lines: float32 phi_hl per level,
    float32 tav of the ERA state, float32 delta_ps / ps_pgw, float32 e_sat chain of RELHUM; 4-D outputs float64.
    Same pass count and error history; PS identical up to one float32 ulp; T, U, V to 1e-9; QV to a few float32 ulp of the
    float32 exp the reference takes (numpy SIMD expf vs device expf) relative to the level's scale."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    nlat, nlon, nlev = shape
    c = _case(nlat, nlon, nlev, seed=seed, dtype=np.float32)
    c['deltas'] = {k: v.astype(delta_dtype) for k, v in c['deltas'].items()}
    got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    # the device holds the deltas in the ERA storage type: the oracle sees the same float32 values
    d32 = {k: v.astype(np.float32) for k, v in c['deltas'].items()}
    want = R.pgw_for_era5_arrays(c['era'], d32, c['delta_times'], c['plev'], c['target_dt'], True)
    assert got['n_iter'] == want['n_iter']
    np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=0, atol=2e-3)
    for k in ('T', 'QV', 'U', 'V', 'RELHUM_pgw'):
        assert got[k].dtype == np.float64 and want[k].dtype == np.float64, k
    for k in ('PS', 'T_SKIN', 'T_SO', 'FR_SEA_ICE'):
        assert got[k].dtype == np.float32 and want[k].dtype == np.float32, k
        np.testing.assert_allclose(got[k], want[k], rtol=1.3e-7, atol=0, equal_nan=True, err_msg=k)
    for k in ('T', 'U', 'V'):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-9, err_msg=k)
    assert _scaled_qv_diff(got['QV'], want['QV']) < 6e-7
    # the float64-arithmetic mode on the same file is measurably further away (that is why this mode exists)
    fast = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, ref_dtype=False)
    assert fast['T'].dtype == np.float32
    d_ref = np.max(np.abs(got['PS'].astype(np.float64) - want['PS']) / want['PS'])
    d_fast = np.max(np.abs(fast['PS'].astype(np.float64) - want['PS']) / want['PS'])
    assert d_ref <= 1.3e-7 and d_ref <= d_fast


def test_reference_dtype_mode_exact_record_and_errors():
    """A time stamp that is a delta record (no time interpolation: the deltas stay float32, functions.py:282-283, and numba
    takes y_hi - y_lo in float32, :575-578) and the data errors of the file path, in reference-dtype mode."""
    import datetime as dt
    from pgw4era5_amd import step_03_apply_to_era as s3, synthetic
    c = synthetic.make_case(6, 10, 40, seed=61, dtype=np.float32, target_dt=dt.datetime(2006, 3, 15, 12))
    got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    want = R.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    assert got['n_iter'] == want['n_iter']
    np.testing.assert_allclose(got['PS'], want['PS'], rtol=1.3e-7)
    for k in ('T', 'U', 'V'):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-9, err_msg=k)
    assert _scaled_qv_diff(got['QV'], want['QV']) < 6e-7
    # surface riders at a record: `delta / 100`, the sea-ice sum and the tos / ts blend are float32 operations in numpy
    # (found by tools/fuzz_parity.py: float64 arithmetic is up to 26 float32 ulp away where sic + delta / 100 cancels)
    np.testing.assert_array_equal(got['FR_SEA_ICE'], want['FR_SEA_ICE'])
    for k in ('T_SKIN', 'T_SO'):
        np.testing.assert_allclose(got[k], want[k], rtol=6e-8, atol=0, equal_nan=True, err_msg=k)
    with pytest.raises(ValueError) as e:
        s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], False)
    assert 'ERA5 top pressure is lower than climate delta top pressure' in str(e.value)
    with pytest.raises(ValueError) as e:
        s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref=100000.0)
    assert 'p_ref locally lies below the surface' in str(e.value)
    with pytest.raises(ValueError):                  # float64 storage has no reference-dtype mode
        c64 = _case(4, 5, 12, seed=5)
        s3.pgw_for_era5_arrays(c64['era'], c64['deltas'], c64['delta_times'], c64['plev'], c64['target_dt'], True, ref_dtype=True)


@pytest.mark.parametrize('shape,seed,label', [((10, 10, 20), 0, 'config 1 (10x10 L20)'),
                                              ((104, 1440, 137), 1, '104-row band of config 2 (0.25 deg L137)')])
def test_float32_file_three_way_record(shape, seed, label):
    """on float32 files, record the pass count and max |dPS| of (a) the reference-dtype oracle = what the
    reference's numpy promotion computes, (b) the float64 oracle on the same values, (c) the HIP float32-storage path in
    both modes.  The numbers go to gpurun_out/f32_three_way.json (DESIGN.md section 2 quotes them)."""
    import json
    import os
    from pgw4era5_amd import step_03_apply_to_era as s3
    nlat, nlon, nlev = shape
    c = _case(nlat, nlon, nlev, seed=seed, dtype=np.float32)
    args = (c['delta_times'], c['plev'], c['target_dt'], True)
    ref = R.pgw_for_era5_arrays(c['era'], c['deltas'], *args)
    era64 = {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v)
             for k, v in c['era'].items()}
    f64 = O.pgw_for_era5_arrays(era64, {k: np.asarray(v, dtype=np.float64) for k, v in c['deltas'].items()}, *args)
    hip_ref = s3.pgw_for_era5_arrays(c['era'], c['deltas'], *args, ref_dtype=True)
    hip_fast = s3.pgw_for_era5_arrays(c['era'], c['deltas'], *args, ref_dtype=False)
    ps_ref = ref['PS'].astype(np.float64)

    def row(name, r):
        return dict(path=name, n_iter=int(r['n_iter']), max_err=[float(x) for x in r['max_err']],
                    max_abs_dPS_vs_reference_dtype=float(np.max(np.abs(np.asarray(r['PS'], dtype=np.float64) - ps_ref))),
                    max_rel_dPS_vs_reference_dtype=float(np.max(np.abs(np.asarray(r['PS'], dtype=np.float64) - ps_ref) / ps_ref)))
    rows = [row('oracle reference-dtype (numpy promotion of the reference)', ref), row('oracle float64', f64),
            row('HIP float32 storage, reference-dtype mode', hip_ref), row('HIP float32 storage, float64 arithmetic (fast)', hip_fast)]
    print('\n' + label)
    for r in rows:
        print('  %-58s n_iter %d  last max|err| %.4f  max|dPS| %.3e Pa (%.2e rel)'
              % (r['path'], r['n_iter'], r['max_err'][-1], r['max_abs_dPS_vs_reference_dtype'], r['max_rel_dPS_vs_reference_dtype']))
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(out_dir):
        path = os.path.join(out_dir, 'f32_three_way.json')
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[label] = rows
        json.dump(rec, open(path, 'w'), indent=1)
    # the reference-dtype mode reproduces the reference's float32 flow: same pass count and error history; PS within a few
    # float32 ulp (where the device log and numpy's log differ in the last float64 bit, a float32 rounding of phi_hl can
    # fall the other way: 0.0078 m2/s2 = one ulp of PS; seen: <= 4 ulp in 150 k columns x 60 levels x 7 passes)
    assert hip_ref['n_iter'] == ref['n_iter']
    assert rows[2]['max_rel_dPS_vs_reference_dtype'] <= 6e-7
    np.testing.assert_allclose(hip_ref['max_err'], ref['max_err'], rtol=0, atol=2e-3)
    # float64 arithmetic (oracle and HIP alike) sits a float32-phi noise floor away from it - on the 0.25 deg band the
    # reference-dtype flow needs one pass more (max|err| of pass 6: 0.1511 against the 0.15 threshold, 0.126 in float64),
    # which moves PS by 1.8e-6: outside north_star's 1e-6, hence the reference-dtype mode
    assert hip_fast['n_iter'] == f64['n_iter']
    assert rows[3]['max_rel_dPS_vs_reference_dtype'] < 3e-6
    assert rows[2]['max_rel_dPS_vs_reference_dtype'] < rows[3]['max_rel_dPS_vs_reference_dtype']


# ------------------------------------------------------------------ ragged / odd shapes, other level sets
@pytest.mark.parametrize('shape', [(7, 13, 21), (3, 5, 9), (1, 3, 6), (2, 2, 5)])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_whole_file_odd_shapes(shape, dtype):
    """Column counts that are not multiples of the vector width (scalar-column code path), level counts
    that are not multiples of the prefetch chunk, single rows / tiny grids."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    nlat, nlon, nlev = shape
    c = _case(nlat, nlon, nlev, seed=50 + nlat * nlon, dtype=dtype)
    got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, ref_dtype=False)
    era64 = {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v)
             for k, v in c['era'].items()}
    want = O.pgw_for_era5_arrays(era64, {k: np.asarray(v, dtype=np.float64) for k, v in c['deltas'].items()},
                                 c['delta_times'], c['plev'], c['target_dt'], True)
    assert got['n_iter'] == want['n_iter']
    tol = 1e-9 if dtype == np.float64 else 1e-6
    for k in ['PS', 'T', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE']:
        np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=1e-5 if (dtype == np.float32 and k in 'UV') else 1e-12,
                                   equal_nan=True, err_msg=k)
    np.testing.assert_allclose(got['QV'], want['QV'], rtol=tol if dtype == np.float64 else 3e-6, atol=1e-18)


@pytest.mark.parametrize('which', ['all_nan', 'only_partial_wave_valid', 'only_partial_wave_nan'])
def test_loop_maximum_with_a_partial_last_wave_and_nan_columns(which):
    """step_03:308 takes the maximum of |phi error| with NaNs skipped (all NaN -> NaN, which ends the loop).  The loop
    kernel reduces per wave; with 5 x 19 = 95 columns the last wave has 31 live lanes.  Columns are switched off by a NaN
    surface geopotential (phi NaN, no error raised): everywhere (the history must read NaN, one pass - an idle lane
    contributing a zero made it 0.0), everywhere but the partial wave, and in the partial wave only (the maximum of the first
    pass is then finite, and the second pass raises like the reference)."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    c = _case(5, 19, 24, seed=91, dtype=np.float64)
    fis = c['era']['FIS'].reshape(-1)
    if which == 'all_nan':
        fis[:] = np.nan
    elif which == 'only_partial_wave_valid':
        fis[:64] = np.nan
    else:
        fis[64:] = np.nan
    args = (c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    if which != 'all_nan':
        # a NaN error makes the column's adjustment, hence its next surface pressure, NaN: pass 2 finds no half level below
        # p_ref there and the reference raises (functions.py:162-165) - on both sides, whichever wave holds the column
        for run in (s3.pgw_for_era5_arrays, O.pgw_for_era5_arrays):
            with pytest.raises(ValueError, match='p_ref locally lies below the surface'):
                run(*args)
        return
    got = s3.pgw_for_era5_arrays(*args)
    want = O.pgw_for_era5_arrays(*args)
    assert got['n_iter'] == want['n_iter']
    np.testing.assert_allclose(np.asarray(got['max_err'])[:got['n_iter']], np.asarray(want['max_err'])[:got['n_iter']], rtol=1e-9,
                               equal_nan=True)
    if which == 'all_nan':                         # the same through the LOCAL form of the loop kernel (p_ref_inp = None)
        loc = s3.pgw_for_era5_arrays(*args, p_ref='local')
        assert loc['n_iter'] == 1 and np.isnan(loc['max_err'][0])
    if which == 'all_nan':
        assert got['n_iter'] == 1 and np.isnan(got['max_err'][0])
    np.testing.assert_allclose(got['PS'], want['PS'], rtol=1e-9, equal_nan=True)


def test_whole_file_plev34_and_exact_month():
    """34 delta levels (the Emon+Amon merge of step_01, Emon_add_top_from_Amon.sh:45,50) and a time stamp
    that hits a delta record exactly (no lerp, functions.py:282-283)."""
    import datetime as dt
    from pgw4era5_amd import step_03_apply_to_era as s3, synthetic
    plev34 = np.concatenate([np.array([100000., 97500, 95000, 92500, 90000, 87500, 85000, 82500, 80000, 77500, 75000,
                                       70000, 65000, 60000, 55000, 50000, 45000, 40000, 35000, 30000, 25000, 22500,
                                       20000, 17500, 15000, 12500, 10000]), synthetic.PLEV19[12:]])
    assert len(plev34) == 34
    c = synthetic.make_case(6, 10, 40, seed=61, plev=plev34, target_dt=dt.datetime(2006, 3, 15, 12))
    got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    want = O.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
    assert got['n_iter'] == want['n_iter']
    for k in ['PS', 'T', 'QV', 'U', 'V']:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12, err_msg=k)


def test_whole_file_errors_reach_python():
    """Data errors inside the fused file path surface as the reference's exceptions."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    c = _case(5, 6, 16, seed=71)
    with pytest.raises(ValueError) as e:                          # model top above delta top, no -t
        s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], False)
    assert 'ERA5 top pressure is lower than climate delta top pressure' in str(e.value)
    bad = {k: v.copy() for k, v in c['deltas'].items()}
    bad['ps_hist'][:, 2, 3] = 50.0                                # HIST surface pressure above the delta top
    with pytest.raises(ValueError) as e:
        s3.pgw_for_era5_arrays(c['era'], bad, c['delta_times'], c['plev'], c['target_dt'], True)
    assert str(e.value) == '' and e.value.column == 2 * 6 + 3
    with pytest.raises(ValueError) as e:                          # p_ref below the surface somewhere
        s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref=100000.0)
    assert 'p_ref locally lies below the surface' in str(e.value)
    with pytest.raises(KeyError):                                 # .sel(plev=p_ref) with a level that is not in the file
        s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref=31000.0)
    era = dict(c['era']); era['PS'] = c['era']['PS'].copy(); era['PS'][0, 1, 1] = np.nan
    with pytest.raises(ValueError):                               # NaN surface pressure: all-NaN p_diff column
        s3.pgw_for_era5_arrays(era, c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)


@pytest.mark.parametrize('opts', [dict(quad=0), dict(full_column=1), dict(force_vec1=1), dict(multipass=0),
                                  dict(multipass=0, full_column=1), dict(quad=0, multipass=0, force_vec1=1),
                                  dict(loop_guess=1), dict(loop_guess=2), dict(loop_guess=5), dict(loop_guess=8),
                                  dict(force_off64=1)])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_kernel_variants_are_bit_identical(opts, dtype):
    """Every selectable variant of the file path (pgw_set_option: pair kernels instead of the quad kernel, full-column
    passes, scalar columns, one launch per loop pass instead of the column-resident multi-pass kernel, 64-bit byte offsets
    - the instantiation arrays of 4 GiB and more take -) produces the same bits as the default: they differ in scheduling
    and addressing, not in arithmetic."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    c = _case(8, 12, 27, seed=81, dtype=dtype)
    a = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, ref_dtype=False)
    old = {k: ctx.set_option(k, v) for k, v in opts.items()}
    try:
        b = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, ref_dtype=False)
        if 'loop_guess' in opts:
            # a first launch of 1, 2, 5 or 8 passes (the file needs 6): continuation launches / speculated passes;
            # afterwards the guess is the file's own pass count
            assert ctx.get_option('loop_guess') == b['n_iter']
            # the launch plan: the guess, clamped to [1, min(8, max_n_iter)], then 2 passes per launch; never more than
            # max_n_iter still allows, never fewer than 1
            import pgw4era5_amd.settings as S
            plan = []
            while sum(plan) < b['n_iter']:
                want = 2 if plan else max(min(opts['loop_guess'], 8, S.max_n_iter), 1)
                plan.append(max(min(want, S.max_n_iter - sum(plan)), 1))
            assert b['passes_launched'] == sum(plan) and (opts['loop_guess'] != 8 or b['passes_launched'] == 8)
    finally:
        for k, v in old.items():
            if k != 'loop_guess':
                ctx.set_option(k, v)
    assert a['n_iter'] == b['n_iter'] and a['max_err'] == b['max_err']
    for k in ['PS', 'T', 'QV', 'U', 'V', 'RELHUM_pgw']:
        if k == 'QV' and dtype == np.float32:
            # the quad kernel writes the final QV of the pure-pressure levels from the fp64 vapour pressure; the pair /
            # full-column variants store the vapour pressure in the storage type first: one float32 rounding apart
            np.testing.assert_allclose(a[k], b[k], rtol=2.5e-7, atol=0, err_msg=k)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------------------------ byte order conversion (NetCDF classic is big-endian)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [1, 3, 4, 1023, 65536 + 5])
def test_byteswap_matches_numpy(dtype, n):
    import ctypes as C
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    rng = np.random.default_rng(n)
    x = rng.normal(size=n).astype(dtype)
    x[0] = np.nan
    d = ctx.to_device(x)
    out = ctx.empty((n,), dtype)
    ctx._check(ctx.lib.pgw_byteswap(ctx.handle, x.itemsize, n, d.ptr, out.ptr))
    np.testing.assert_array_equal(out.numpy().view(np.uint8), x.byteswap().view(np.uint8))
    ctx._check(ctx.lib.pgw_byteswap(ctx.handle, x.itemsize, n, out.ptr, out.ptr))               # in place, back again
    np.testing.assert_array_equal(out.numpy().view(np.uint8), x.view(np.uint8))
    if n > 1:                                                                                     # element-aligned, not 16 B aligned
        ctx._check(ctx.lib.pgw_byteswap(ctx.handle, x.itemsize, n - 1, d.ptr + x.itemsize, out.ptr + x.itemsize))
        np.testing.assert_array_equal(out.numpy()[1:].view(np.uint8), x[1:].byteswap().view(np.uint8))
    # DeviceArray.copy_from of an array in the file's byte order, download_foreign back
    be = x.astype(x.dtype.newbyteorder('>'))
    d2 = ctx.empty((n,), dtype).copy_from(be)
    np.testing.assert_array_equal(d2.numpy().view(np.uint8), x.view(np.uint8))
    host = np.zeros(d2.nbytes + 3, dtype=np.uint8)
    back = d2.download_foreign(host)
    ctx.sync()
    assert back.dtype == be.dtype
    np.testing.assert_array_equal(back.view(np.uint8), be.view(np.uint8))
    with pytest.raises(ValueError):
        ctx._check(ctx.lib.pgw_byteswap(ctx.handle, 2, n, d.ptr, out.ptr))


def test_file_with_two_time_steps_fails_like_the_reference():
    """The deltas are interpolated to one instant, so a file with two time steps fails in the reference at
    functions.py:457-459 (oracle: same message); function-level calls with ntime > 1 are legal and must index the
    time axis correctly."""
    from pgw4era5_amd import step_03_apply_to_era as s3, functions as F
    cs = [_case(5, 6, 12, seed=s) for s in (1, 2)]
    era = dict(cs[0]['era'])
    for k, v in era.items():
        if isinstance(v, np.ndarray) and v.ndim >= 3:
            era[k] = np.concatenate([c['era'][k] for c in cs], axis=0)
    c = cs[0]
    for run in (O.pgw_for_era5_arrays, s3.pgw_for_era5_arrays):
        with pytest.raises(ValueError) as e:
            run(era, c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
        assert str(e.value) == 'Time dimension of input files is inconsistent!'
    # function level, ntime = 2: every time slice equals the single-time result
    pa_hl, pa = F.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    rh = F.specific_to_relative_humidity(era['QV'], pa, era['T'])
    phi = F.integ_geopot(pa_hl, era['FIS'], era['T'], era['QV'], era['level1'], 30000.0)
    src_p = np.broadcast_to(np.asarray(c['plev'])[::-1][None, :, None, None], (2, len(c['plev'])) + era['PS'].shape[1:]).copy()
    var = np.random.default_rng(0).normal(size=src_p.shape)
    itp = F.interp_logp_4d(var, src_p, pa, 'constant')
    for t, ct in enumerate(cs):
        e1 = ct['era']
        hl1, pa1 = F.hybrid_pressure(e1['ak'], e1['bk'], e1['PS'])
        np.testing.assert_array_equal(pa_hl[t:t + 1], hl1)
        np.testing.assert_array_equal(rh[t:t + 1], F.specific_to_relative_humidity(e1['QV'], pa1, e1['T']))
        np.testing.assert_array_equal(phi[t:t + 1], F.integ_geopot(hl1, e1['FIS'], e1['T'], e1['QV'], e1['level1'], 30000.0))
        np.testing.assert_array_equal(itp[t:t + 1], F.interp_logp_4d(var[t:t + 1], src_p[t:t + 1], pa1, 'constant'))
    np.testing.assert_allclose(phi, O.integ_geopot(pa_hl, era['FIS'], era['T'], era['QV'], era['level1'], 30000.0), rtol=1e-12)


# ------------------------------------------------------------------ step_02 smoothing (functions.py:603-740)
def test_harmonic_smoothing_golden_and_oracle(F, golden_harmonic):
    """pgw_harmonic_smooth against the reference's own outputs (golden vectors) and the oracle on 3-D / 4-D blocks.
    Tolerances: fp64 series 1e-12 of the series' scale (summation order: sequential on the GPU, BLAS dot / pairwise
    mean in numpy); float32 series 1e-6 of the scale - the reference forms the mean of a float32 series in float32
    (numpy keeps the dtype), this build in fp64."""
    g, meta = golden_harmonic
    for lt in (365, 366, 360, 8, 9):
        ts, want = g['ts64_%d' % lt], g['sm64_%d' % lt]
        for x, w in zip(ts, want):
            got = F.harmonic_ac_analysis(x)
            assert got.dtype == np.float64
            np.testing.assert_allclose(got, w, rtol=0, atol=1e-12 * np.abs(x).max())
        cube = np.ascontiguousarray(g['ts32_%d' % lt].T.reshape(lt, 2, 3))                  # (time, y, x) float32
        sm = F.smooth_annual_cycle(cube)
        assert sm.dtype == np.float32 and sm.shape == cube.shape
        np.testing.assert_allclose(sm.reshape(lt, 6).T, g['sm32_%d' % lt], rtol=0, atol=1e-6 * np.abs(cube).max())
    out = F.harmonic_ac_analysis(g['nan_in'])
    assert np.isnan(out).all() and out.shape == g['nan_in'].shape
    with pytest.raises(ValueError) as e:
        F.harmonic_ac_analysis(np.arange(7.0))
    assert 'Whooops' in str(e.value)
    with pytest.raises(ValueError):
        F.smooth_annual_cycle(np.zeros((8, 3)))
    rng = np.random.default_rng(5)
    for shape in [(365, 3, 7, 11), (366, 5, 300), (8, 1, 1, 1)]:
        x = rng.normal(1.0, 2.0, shape)
        x[3, ..., 0] = np.nan                                   # NaN columns come back all NaN, the others untouched by them
        got = F.smooth_annual_cycle(x)
        np.testing.assert_allclose(got, O.filter_data_array(x), rtol=0, atol=1e-12 * 10, equal_nan=True)


def test_shared_divisor_is_ieee_division():
    """SharedDivisor (reciprocal once + three instructions per quotient) must give the correctly rounded IEEE
    quotient - the same bits as numpy's `/` - over the operand ranges it is used with (grid spacings, ln-pressure
    intervals, field differences) and far beyond; NaN numerators propagate."""
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    rng = np.random.default_rng(123)
    n = 1 << 21
    num = rng.normal(size=n) * 10.0 ** rng.uniform(-12, 12, n)
    den = rng.uniform(0.5, 2.0, n) * 10.0 ** rng.uniform(-8, 8, n) * rng.choice([-1.0, 1.0], n)
    num[:8] = [0.0, -0.0, np.nan, 1.0, 3.0, 1e-200, 1e200, 7.0]
    den[:8] = [3.0, 3.0, 2.0, 3.0, 1.0, 1e-3, 1e3, 0.1]
    # mantissa patterns that stress the rounding: numerators just around representable quotient boundaries
    q = rng.uniform(1, 2, 4096)
    d = rng.uniform(1, 2, 4096)
    num[100:100 + 4096] = np.nextafter(q * d, np.inf)
    den[100:100 + 4096] = d
    den[10000:400000] = 100.0                                   # the compile-time divisor of rh_to_e (hur / 100)
    num[10000:200000] = rng.uniform(-50, 200, 190000)
    dn, dd = ctx.to_device(num), ctx.to_device(den)
    out = ctx.empty((n,), np.float64)
    ctx._check(ctx.lib.pgw_test_shared_div(ctx.handle, n, dn.ptr, dd.ptr, out.ptr))
    got = out.numpy()
    with np.errstate(all='ignore'):
        want = num / den
    np.testing.assert_array_equal(got, want)          # equal doubles = equal bits, up to the sign of a zero quotient and NaN payloads


def test_reference_mode_esat_f32_fast_path_is_the_literal_expression():
    """Reference-dtype mode, RELHUM of the float32 ERA state (step_03:91-94 through functions.py:58-116 on float32 arrays):
    the quad kernel evaluates ONE phase of e_sat (alpha in {0, 1} makes the other term an exact zero), with scale-free
    float32 / float64 divisions and the library's expf arithmetic without its range selects.  It must give the bits of the
    expression as written - both phases, IEEE divisions, expf() - for every float32 temperature (the mixed range, below
    60 K, NaN and infinities take the literal code), and the literal e_sat must be numpy's float32 evaluation to 4 ulp
    (the device expf against numpy's SIMD float32 exp, each within a few ulp of the exact value, and alpha's weights in
    the mixed range; tests/golden/ref_leaf_f32_vectors.npz pins the dtype flow itself)."""
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    rng = np.random.default_rng(77)
    n = 1 << 21
    ta = rng.uniform(150.0, 340.0, n).astype(np.float32)
    ta[:200000] = rng.uniform(249.0, 274.5, 200000).astype(np.float32)             # around both phase limits
    edge = np.array([273.16, 250.16, 60.0, 32.19, -0.7, 0.0, 1e4, 3e38, np.inf, -np.inf, np.nan, 40.0, 59.999, 60.001],
                    np.float32)
    edge = np.concatenate([edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))])
    ta[200000:200000 + edge.size] = edge
    ta[300000:310000] = rng.uniform(-50.0, 70.0, 10000).astype(np.float32)         # unphysically cold
    hus = rng.uniform(0.0, 0.03, n).astype(np.float32)
    hus[:16] = [0.0, 1e-7, 1e-30, 0.5, 1.0, np.nan, -1e-5, 3e-6, 0.02, 0.03, 1e-3, 1e-4, 1e-5, 1e-6, 0.01, 0.005]
    pa = rng.uniform(1.0, 1.08e5, n)
    d_ta, d_hus, d_pa = ctx.to_device(ta, np.float32), ctx.to_device(hus, np.float32), ctx.to_device(pa)
    out, lit = ctx.empty((n,), np.float64), ctx.empty((n,), np.float64)
    es, es_lit = ctx.empty((n,), np.float32), ctx.empty((n,), np.float32)
    ctx._check(ctx.lib.pgw_test_rh_f32(ctx.handle, n, d_hus.ptr, d_pa.ptr, d_ta.ptr, out.ptr, lit.ptr, es.ptr, es_lit.ptr))
    g_es, w_es = es.numpy(), es_lit.numpy()
    np.testing.assert_array_equal(g_es.view(np.uint32)[~np.isnan(w_es)], w_es.view(np.uint32)[~np.isnan(w_es)])
    assert np.isnan(g_es[np.isnan(w_es)]).all()
    phys = np.isfinite(ta) & (ta > 60.0)
    got, want = out.numpy(), lit.numpy()
    np.testing.assert_array_equal(got[phys], want[phys])                           # NaN == NaN positions included
    # the literal e_sat against numpy's float32 evaluation of functions.py:74-105
    with np.errstate(all='ignore'):
        t = ta[phys]
        f32 = np.float32
        ew = f32(611.21) * np.exp(f32(17.502) * (t - f32(273.16)) / (t - f32(32.19)))
        ei = f32(611.21) * np.exp(f32(22.587) * (t - f32(273.16)) / (t - f32(-0.7)))
        alpha = np.where(t >= f32(273.16), f32(1), np.where(t <= f32(250.16), f32(0), ((t - f32(250.16)) / f32(23.0)) ** 2)).astype(f32)
        ref = alpha * ew + (f32(1) - alpha) * ei
    ok = np.isfinite(ref) & (ref > 1e-30)
    ulp = np.abs(w_es[phys][ok].astype(np.float64) - ref[ok].astype(np.float64)) / np.spacing(ref[ok]).astype(np.float64)
    assert ok.sum() > 2000000 and ulp.max() <= 4.0, ulp.max()
    for x in (d_ta, d_hus, d_pa, out, lit, es, es_lit):
        x.free()


def test_device_exp_is_library_exp():
    """pgw_exp (explicit-FMA restatement of the device library's exp, used by every e_sat evaluation) gives the
    library's bits over the arguments of the path and far beyond, incl. overflow / underflow / NaN / inf, and is
    within 1 ulp of numpy."""
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    rng = np.random.default_rng(321)
    x = np.concatenate([rng.uniform(-40, 12, 1 << 20),          # 17.5 (T - T0) / (T - 32), 22.6 (T - T0) / (T + 0.7)
                        rng.uniform(-760, 720, 1 << 18),
                        np.array([0.0, -0.0, 1.0, -1.0, 709.78, 709.79, 710.0, 1024.0, 1025.0, -745.0, -745.2, -1075.0, -1076.0,
                                  np.inf, -np.inf, np.nan, 1e-300, -1e-300, 5e-324])])
    n = x.size
    dx = ctx.to_device(x)
    out, ref = ctx.empty((n,), np.float64), ctx.empty((n,), np.float64)
    ctx._check(ctx.lib.pgw_test_exp(ctx.handle, n, dx.ptr, out.ptr, ref.ptr))
    got, lib = out.numpy(), ref.numpy()
    np.testing.assert_array_equal(got, lib)
    with np.errstate(all='ignore'):
        want = np.exp(x)
    fin = np.isfinite(want) & (want > 1e-300)
    ulp = np.abs(got[fin] - want[fin]) / np.spacing(want[fin])
    assert ulp.max() <= 1.0, ulp.max()
    assert np.isnan(got[np.isnan(x)]).all() and got[x == np.inf][0] == np.inf and got[x == -np.inf][0] == 0.0


@pytest.mark.parametrize('rows,ncol', [(1, 5), (2, 130), (5, 300), (8, 128)])
@pytest.mark.parametrize('ns,nd', [(1, 1), (4, 4), (0, 2), (3, 1)])
def test_placement_probe_moves_the_bytes_it_reports(rows, ncol, ns, nd):
    """pgw_placement_probe (the column kernels' access pattern with no arithmetic; measurement of where the arrays lie in
    HBM, no counterpart in the reference): every element of every write stream is the sum of the read streams at its
    place - odd row counts, a partial last block, no read streams - and the rate comes back positive."""
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    rng = np.random.default_rng(rows * 1000 + ncol)
    src_h = [rng.normal(size=(1, rows, 1, ncol)) for _ in range(ns)]
    src = [ctx.to_device(x) for x in src_h]
    dst = [ctx.to_device(np.full((1, rows, 1, ncol), -7.0)) for _ in range(nd)]
    g = ctx.placement_probe(src, dst, reps=2)
    assert g > 0.0
    want = np.zeros((1, rows, 1, ncol))
    for x in src_h:                                 # the kernel's order of additions: stream 0 first, from 0.0
        want = want + x
    for d in dst:
        np.testing.assert_array_equal(d.numpy(), want)
    for x, d in zip(src_h, src):                    # read streams untouched
        np.testing.assert_array_equal(d.numpy(), x)
    with pytest.raises(ValueError):
        ctx.placement_probe([dst[0]] * 5, dst)                                      # more than 4 read streams


def test_an_adopted_workspace_changes_nothing_in_the_results():
    """pgw_ws_adopt: the vapour-pressure workspace of the file path in a buffer the caller allocated (so that the host layer
    can choose its place in HBM) - same bits as with the library's own; a buffer that is too small is replaced by the
    library, not written past."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    c = _case(nlat=6, nlon=11, nlev=20, seed=5)
    args = (c['delta_times'], c['plev'], c['target_dt'])
    ctx = default_context()
    want = s3.pgw_for_era5_arrays(c['era'], c['deltas'], *args, ignore_top_pressure_error=True)
    for nbytes in (c['era']['T'].size * 8, c['era']['T'].size * 8 + 4096, 64):
        ws = ctx.empty((nbytes // 8,), np.float64)
        ctx.ws_adopt(0, ws)
        assert ws._owner is None                    # the library's now
        with pytest.raises(ValueError):
            ctx.ws_adopt(0, ws)                     # not ours to hand over twice
        got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], *args, ignore_top_pressure_error=True)
        assert got['n_iter'] == want['n_iter']
        for k in ('PS', 'T', 'QV', 'U', 'V'):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    ctx._check(ctx.lib.pgw_ws_adopt(ctx.handle, 0, None, 0))        # release
    with pytest.raises(ValueError):
        ctx._check(ctx.lib.pgw_ws_adopt(ctx.handle, 9, None, 0))


def test_spread_pool_stock_alternation_and_fallbacks(monkeypatch):
    """device.SpreadPool / Context.enable_placement / Context.level_array (placement of the level arrays over the card's
    memory regions; no counterpart in the reference, no influence on results): arrays below the probe size are plain stock;
    `take` alternates the two stock lists, serves smaller requests as views, refuses larger ones, and falls back to plain
    memory when the stock is used up; `PGW_PLACEMENT=plain` turns the whole thing off."""
    from pgw4era5_amd.device import Context, SpreadPool
    ctx = Context(0)
    try:
        pool = SpreadPool(ctx, 4096, 5)
        assert pool.info['classes'] == 1 and pool.info['kept'] == 5 and len(pool.stock[0]) == 5 and pool.stock[1] == []
        pool.stock[1] = [pool.stock[0].pop(), pool.stock[0].pop()]                  # pretend two lie outside the reference's stretch
        for a in pool.stock[1]:
            a._cls = 1
        pool.info['classes'] = 2
        got = [pool.take((8, 64), np.float64) for _ in range(5)]
        assert [g.placement_class for g in got] == [0, 1, 0, 1, 0]
        assert len(set(g.ptr for g in got)) == 5
        extra = pool.take((2, 3), np.float32)                                       # stock used up: plain memory
        assert extra.placement_class is None and extra.ptr not in [g.ptr for g in got]
        with pytest.raises(ValueError):
            pool.take((4097,), np.uint8 if False else np.float64)
        x = np.arange(512, dtype=np.float64).reshape(8, 64)
        np.testing.assert_array_equal(got[1].copy_from(x).numpy(), x)               # a view of a stock array is an ordinary array
        assert pool.take_owner() is None
        ptr1 = got[1].ptr
        del got[1]                                                                  # the last view gone: back into the stock, same class
        import gc
        gc.collect()                                                                # (an owning array refers to itself)
        assert [a.ptr for a in pool.stock[1]] == [ptr1] and pool.stock[0] == []
        again = pool.take((8, 64), np.float64, cls=1)
        assert again.ptr == ptr1 and again.placement_class == 1
        # the context-level switches
        monkeypatch.setenv('PGW_PLACEMENT', 'plain')
        assert ctx.enable_placement(1 << 16, 3) is None and getattr(ctx, '_spread', None) is None
        monkeypatch.setenv('PGW_PLACEMENT', 'sideways')
        with pytest.raises(ValueError):
            ctx.enable_placement(1 << 16, 3)
        monkeypatch.setenv('PGW_PLACEMENT', 'spread')
        info = ctx.enable_placement(1 << 16, 3)
        assert info['kept'] == 3 and ctx.enable_placement(1 << 16, 3) is info       # idempotent per size
        a = ctx.level_array((1, 2, 64, 64), np.float64)                             # 64 KiB: the pool's size
        b = ctx.level_array((1, 2, 64, 64), np.float32)                             # half of it: still a level field
        c = ctx.level_array((16,), np.float64)                                      # a small array: plain
        assert a.placement_class == 0 and b.placement_class == 0 and c.placement_class is None
    finally:
        ctx.close()


def test_spread_pool_draw_with_probes_keeps_what_was_asked_for():
    """The drawing loop with real probes (32 MiB arrays: above the probe size; a budget of 1 GiB, so no spacer fits): whatever
    the card answers - one class or two - `count` distinct usable arrays come back and the rest is freed."""
    from pgw4era5_amd.device import Context, SpreadPool
    ctx = Context(0)
    try:
        live0 = ctx._live
        pool = SpreadPool(ctx, 32 << 20, 6, budget_bytes=1 << 30)
        assert pool.info['kept'] == 6 and pool.info['classes'] in (1, 2) and pool.info['drawn_GB'] <= 1.08
        arrs = [pool.take((1, 4, 1024, 1024), np.float64) for _ in range(6)]
        assert len(set(a.ptr for a in arrs)) == 6
        assert ctx._live - live0 == 6 * (32 << 20)                                   # candidates beyond the stock were freed
        for i, a in enumerate(arrs):
            ctx._check(ctx.lib.pgw_memset(ctx.handle, a.ptr, i, a.nbytes))
        for i, a in enumerate(arrs):
            assert np.all(a.numpy().view(np.uint8) == i)
    finally:
        ctx.close()


def test_whole_file_results_do_not_depend_on_placement():
    """The same file through the process-wide context before and after `enable_placement` (level arrays and the library's
    vapour-pressure workspace from the pool): identical bits."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    c = _case(nlat=6, nlon=11, nlev=20, seed=8)
    args = (c['delta_times'], c['plev'], c['target_dt'])
    want = s3.pgw_for_era5_arrays(c['era'], c['deltas'], *args, ignore_top_pressure_error=True)
    ctx = default_context()
    info = ctx.enable_placement(c['era']['T'].size * 8, 9)
    assert info is None or info['kept'] >= 9        # >: a driver test before this one has set the process-wide pool up already
    got = s3.pgw_for_era5_arrays(c['era'], c['deltas'], *args, ignore_top_pressure_error=True)
    assert got['n_iter'] == want['n_iter']
    for k in ('PS', 'T', 'QV', 'U', 'V'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_an_allocation_that_does_not_fit_leaves_the_context_usable():
    """pgw_malloc of more than the card has: PGWHipError, and no sticky HIP error left behind - the next kernel launch on the
    context succeeds (the placement draw relies on this when its budget meets a busy card)."""
    from pgw4era5_amd import _lib
    from pgw4era5_amd.device import Context
    ctx = Context(0)
    try:
        _free, total = ctx.mem_info()
        with pytest.raises(_lib.PGWHipError):
            ctx.empty((total // 8 + (1 << 28),), np.float64)
        x = np.arange(1024, dtype=np.float64)
        d = ctx.to_device(x)
        out = ctx.empty((1024,), np.float64)
        ctx._check(ctx.lib.pgw_byteswap(ctx.handle, 8, 1024, d.ptr, out.ptr))
        np.testing.assert_array_equal(out.numpy().view(np.uint8), x.byteswap().view(np.uint8))
    finally:
        ctx.close()
