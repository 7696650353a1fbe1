#!/usr/bin/env python
"""Randomised parity sweep of the function-level entries (the `functions.py` mirror) against the oracles:
interp_logp_4d in all four modes (against the serial C column loops, oracle/pgw_oracle_c.c: pinned by the reference's own
vectors), vert_interp_delta with and without the surface insertion, integ_geopot with a scalar and a per-column p_ref and
the humidity pair (both over 1..3 time steps, float32 storage on ~30 % of the cases: the fp64 oracle on the stored values,
rounded once), regrid_field on random source / target grids (periodic or not, pole rows or not, target longitudes in
-180..180 or 0..360), smooth_annual_cycle on random record counts.  Errors must agree as well.
--dtype-flow reference: settings.function_dtype_flow = 'reference' instead - every case draws a random float32 / float64 mix
of its operands and is checked against oracle/pgw_oracle_refdtype.py (result dtype, values, errors): the humidity pair and
leaves, integ_geopot, interp_logp_4d, vert_interp_delta, time_lerp and integrate_tos.  Without the option the tool draws
exactly the cases it always drew.
Test infrastructure (imports oracle/).  usage: python tools/fuzz_functions.py [--cases 400] [--seed 0] [--dtype-flow reference]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from pgw4era5_amd import functions as F, synthetic
from oracle import pgw_oracle as O, pgw_oracle_c as C


def both(hip, ora):
    """Run both sides; returns (got, want, note).  An exception on one side only is a failure."""
    e1 = e2 = None
    got = want = None
    try:
        got = hip()
    except Exception as e:                      # noqa: BLE001
        e1 = e
    try:
        want = ora()
    except Exception as e:                      # noqa: BLE001
        e2 = e
    if e1 is None and e2 is None:
        return got, want, None
    if e1 is not None and e2 is not None:
        # the oracle's messages are the first sentence of the reference's; the product carries the full text
        if type(e1) is type(e2) and (str(e1) == str(e2) or not str(e2) or str(e1).startswith(str(e2).rstrip('.!'))):
            return None, None, 'both raise'
        return None, None, 'FAIL different errors: %s: %s / %s: %s' % (type(e1).__name__, e1, type(e2).__name__, e2)
    return None, None, 'FAIL one side raises: HIP %r / oracle %r' % (e1, e2)


def close(got, want, rtol, atol):
    return bool(np.allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=rtol, atol=atol, equal_nan=True))


def case_interp(rng):
    nt, S, N, nlat, nlon = int(rng.integers(1, 3)), int(rng.integers(2, 24)), int(rng.integers(1, 50)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
    sp = np.sort(rng.uniform(50., 1.05e5, (nt, S, nlat, nlon)), axis=1)
    tp = np.sort(rng.uniform(20., 1.09e5, (nt, N, nlat, nlon)), axis=1)
    var = rng.normal(size=(nt, S, nlat, nlon))
    mode = str(rng.choice(['off', 'linear', 'constant', 'nan']))
    r = rng.random()
    if mode == 'off' and r < 0.8:
        tp = np.clip(tp, sp[:, :1], sp[:, -1:])                              # in range: no error
    if r < 0.3 and N > 1:
        k = int(rng.integers(0, N)); s = int(rng.integers(0, S))
        tp[:, k] = sp[:, s]                                                  # exact hits (may unsort a column: allowed inside)
        if tp[0, -1, 0, 0] < tp[0, 0, 0, 0]:
            tp = np.sort(tp, axis=1)
    if rng.random() < 0.15:
        var[0, int(rng.integers(0, S)), 0, 0] = np.nan
    if rng.random() < 0.05:
        sp[0, :, 0, 0] = sp[0, ::-1, 0, 0]                                   # descending source column -> ValueError
    f32 = rng.random() < 0.3                                                 # float32 storage: float64 arithmetic on the stored values
    if f32:
        var, sp, tp = var.astype(np.float32), sp.astype(np.float32), tp.astype(np.float32)
    got, want, note = both(lambda: F.interp_logp_4d(var, sp, tp, mode), lambda: C.interp_logp_4d(var, sp, tp, mode))
    if note:
        return 'interp_' + mode, note
    if f32 and got.dtype != np.float32:
        return 'interp_' + mode, 'FAIL dtype %s' % got.dtype
    # the device logarithm is within 1 ulp of numpy's: 1e-13 of a slope of O(1e2) per unit ln p
    return 'interp_' + mode, 'ok' if close(got, want, *((2e-6, 2e-6) if f32 else (1e-9, 1e-9))) else 'FAIL values'


def case_vert(rng):
    nlat, nlon, N = int(rng.integers(1, 6)), int(rng.integers(1, 9)), int(rng.integers(2, 40))
    keep = np.ones(19, dtype=bool)
    if rng.random() < 0.5:
        keep[rng.choice(np.arange(1, 18), size=int(rng.integers(1, 10)), replace=False)] = False
    plev = synthetic.PLEV19[keep]
    S = len(plev)
    delta = rng.normal(size=(1, S, nlat, nlon))
    tp = np.sort(rng.uniform(120., 1.06e5, (1, N, nlat, nlon)), axis=1)
    with_sfc = rng.random() < 0.6
    dsfc = rng.normal(size=(1, nlat, nlon)) if with_sfc else None
    psh = rng.uniform(4.0e4, 1.06e5, (1, nlat, nlon)) if with_sfc else None
    if with_sfc and rng.random() < 0.1:
        psh[0, 0, 0] = 50.0                                                  # below the delta top -> ValueError()
    ignore = rng.random() < 0.8
    if rng.random() < 0.2:
        tp[0, 0] = 30.0                                                      # above the delta top: error unless ignored
        tp = np.sort(tp, axis=1)
    f32 = rng.random() < 0.3
    if f32:
        delta, tp = delta.astype(np.float32), tp.astype(np.float32)
        if with_sfc:
            dsfc, psh = dsfc.astype(np.float32), psh.astype(np.float32)
    got, want, note = both(lambda: F.vert_interp_delta(delta, tp, dsfc, psh, ignore, plev=plev),
                           lambda: O.vert_interp_delta(delta, plev, tp, dsfc, psh, ignore))
    if note:
        return 'vert_interp_delta', note
    return 'vert_interp_delta', 'ok' if close(got, want, *((2e-6, 2e-6) if f32 else (1e-9, 1e-9))) else 'FAIL values'


def _storage(rng):
    """(ntime, storage dtype) of a function-level case: 1..3 time steps, float32 on ~30 % of the cases."""
    return int(rng.integers(1, 4)), (np.float32 if rng.random() < 0.3 else np.float64)


def case_geopot(rng):
    nt, dt = _storage(rng)
    nlat, nlon, nlev, seed = int(rng.integers(1, 7)), int(rng.integers(1, 9)), int(rng.integers(6, 40)), int(rng.integers(0, 1 << 30))
    # time steps: synthetic cases of consecutive seeds on one grid (ak / bk depend on nlev only)
    cs = [synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=seed + k, dtype=dt)['era'] for k in range(nt)]
    era = {k: np.concatenate([c[k] for c in cs]) for k in ('PS', 'FIS', 'T', 'QV')}
    ak, bk = cs[0]['ak'], cs[0]['bk']
    pa_hl = O.hybrid_pressure(ak, bk, era['PS'].astype(np.float64))[0].astype(dt)
    level1 = np.arange(1, len(ak) + 1)
    r = rng.random()
    if r < 0.5:
        p_ref = float(rng.choice([30000.0, 50000.0, 70000.0, 20000.0]))
    elif r < 0.9:
        p_ref = rng.uniform(1.0e4, 0.9 * era['PS'].min(), era['PS'].shape).astype(dt)
    else:
        p_ref = 2.0e5                                                        # below the surface -> ValueError
    f64 = {k: v.astype(np.float64) for k, v in era.items()}                # the oracle: fp64 on the stored values
    got, want, note = both(lambda: F.integ_geopot(pa_hl, era['FIS'], era['T'], era['QV'], level1, p_ref),
                           lambda: O.integ_geopot(pa_hl.astype(np.float64), f64['FIS'], f64['T'], f64['QV'], level1,
                                                  np.asarray(p_ref, dtype=np.float64)))
    if note:
        return 'integ_geopot', note
    if got.dtype != dt:
        return 'integ_geopot', 'FAIL dtype %s' % got.dtype
    # float32: the fp64 result rounded once (plus the fp64 differences, ~1e-13)
    return 'integ_geopot', 'ok' if close(got, want, *((2.0 ** -23, 0) if dt == np.float32 else (1e-11, 1e-6))) else 'FAIL values'


def case_humidity(rng):
    nt, dt = _storage(rng)
    shp = (nt, int(rng.integers(1, 12)), int(rng.integers(1, 6)), int(rng.integers(1, 9)))
    ta = rng.uniform(185.0, 320.0, shp)
    ta.reshape(-1)[: min(3, ta.size)] = [273.16, 250.16, 260.0][: min(3, ta.size)]
    pa = rng.uniform(1.0, 1.05e5, shp)
    hus = 10.0 ** rng.uniform(-7, -1.7, shp)
    hur = rng.uniform(-5.0, 120.0, shp)
    ta, pa, hus, hur = (x.astype(dt).astype(np.float64) for x in (ta, pa, hus, hur))      # the stored values, in fp64
    tol = (2.0 ** -23, 0) if dt == np.float32 else (1e-12, 0)
    got, want, note = both(lambda: F.specific_to_relative_humidity(hus.astype(dt), pa.astype(dt), ta.astype(dt)),
                           lambda: O.specific_to_relative_humidity(hus, pa, ta))
    if note or got.dtype != dt or not close(got, want, *tol):
        return 'humidity', note or 'FAIL q->rh (%s)' % got.dtype
    got, want, note = both(lambda: F.relative_to_specific_humidity(hur.astype(dt), pa.astype(dt), ta.astype(dt)),
                           lambda: O.relative_to_specific_humidity(hur, pa, ta))
    if note:
        return 'humidity', note
    if got.dtype != dt:
        return 'humidity', 'FAIL rh->q dtype %s' % got.dtype
    return 'humidity', 'ok' if close(got, want, tol[0], 1e-300 if dt == np.float64 else 0) else 'FAIL rh->q'


def case_regrid(rng):
    nlat_s, nlon_s = int(rng.integers(4, 40)), int(rng.integers(6, 90))
    nlat_t, nlon_t = int(rng.integers(2, 60)), int(rng.integers(2, 400))
    periodic = rng.random() < 0.75
    polar = rng.random() < 0.7
    x = (np.arange(nlat_s) + 0.5) / nlat_s
    src_lat = (-90.0 + 180.0 * x) * (1 - 0.3 / nlat_s)
    if periodic:
        src_lon = np.arange(nlon_s) * (360.0 / nlon_s)
        targ_lon = np.arange(nlon_t) * (360.0 / nlon_t) - (180.0 if rng.random() < 0.5 else 0.0)
    else:
        src_lon = np.linspace(-30.0, 60.0, nlon_s)
        targ_lon = np.linspace(-29.0 if rng.random() < 0.9 else -35.0, 58.0, nlon_t)    # -35: outside -> ValueError
    if polar:
        targ_lat = np.linspace(-90.0, 90.0, nlat_t)
    else:
        targ_lat = np.linspace(src_lat[0] + 0.1, src_lat[-1] - 0.1, nlat_t)
    if rng.random() < 0.2:
        targ_lat = targ_lat[::-1].copy()
    f = rng.normal(size=(int(rng.integers(1, 4)), int(rng.integers(1, 4)), nlat_s, nlon_s))
    if rng.random() < 0.3:
        f[0, 0, int(rng.integers(0, nlat_s)), int(rng.integers(0, nlon_s))] = np.nan
    if rng.random() < 0.25:                        # GCM latitudes north -> south: flipped like functions.py:822-829 (the pole
        src_lat = src_lat[::-1].copy()             # rows then depend on the sign of dlat_gcm, taken BEFORE the flip, :779)
        f = np.ascontiguousarray(f[..., ::-1, :])
    f32 = rng.random() < 0.3
    if f32:
        f = f.astype(np.float32)
    got, want, note = both(lambda: F.regrid_field(f, src_lat, src_lon, targ_lat, targ_lon),
                           lambda: O.regrid_lat_lon(f.astype(np.float64), src_lat, src_lon, targ_lat, targ_lon))
    if note:
        return 'regrid', note
    return 'regrid', 'ok' if close(got, want, *((1e-6, 1e-6) if f32 else (1e-12, 1e-13))) else 'FAIL values'


def case_smooth(rng):
    nt = int(rng.choice([8, 9, 12, 360, 365, 366, int(rng.integers(7, 400))]))
    x = rng.normal(size=(nt, int(rng.integers(1, 4)), int(rng.integers(1, 5)), int(rng.integers(1, 7))))
    if rng.random() < 0.3:
        x[int(rng.integers(0, nt)), 0, 0, 0] = np.nan
    got, want, note = both(lambda: F.smooth_annual_cycle(x), lambda: O.filter_data_array(x))
    if note:
        return 'smooth', note
    return 'smooth', 'ok' if close(got, want, 1e-11, 1e-12) else 'FAIL values'


def case_ocean(rng):
    """NaN-ignoring Gaussian-kernel interpolation from a curvilinear ocean grid (functions.py:900-1060; parity unpinned:
    the oracle restates the published VTK / Vincenty formulas) on small random grids, radii and sharpness values."""
    oc = synthetic.make_ocean_grid_case(nj=int(rng.integers(8, 22)), ni=int(rng.integers(10, 30)), ntime=int(rng.integers(1, 4)),
                                        seed=int(rng.integers(0, 1 << 30)), land_patches=int(rng.integers(0, 4)))
    nlat, nlon = int(rng.integers(5, 14)), int(rng.integers(6, 21))
    lat = np.linspace(-90.0, 90.0, nlat)
    lon = np.arange(nlon) * (360.0 / nlon)
    land = (rng.uniform(size=(nlat, nlon)) > 0.8).astype(np.float64)
    R, sh = float(rng.uniform(0.8e6, 4.0e6)), float(rng.choice([1.0, 3.0, 4.0]))
    got = F.gauss_interp_fields(land, lat, lon, oc['latitude'], oc['longitude'], list(oc['values']), R, sh)
    for m in range(len(oc['values'])):
        try:
            want = O.nan_ignoring_interp(land, lat, lon, oc['latitude'], oc['longitude'], oc['values'][m], R, sh)
        except ValueError as e:
            if 'outside this oracle' in str(e):          # Vincenty's inverse iteration near antipodal points
                return 'ocean', 'both raise'
            raise
        if not close(got[m], want, 1e-9, 0):
            return 'ocean', 'FAIL values (month %d)' % m
    return 'ocean', 'ok'


# ---- settings.function_dtype_flow = 'reference': random dtype mixes against the reference-dtype oracle --------------------
EXP_F32 = 4 * 2.0 ** -23           # device expf against numpy's float32 exp


def _dt(rng):
    return np.float32 if rng.random() < 0.5 else np.float64


def _verdict(name, got, want, rtol, atol=0.0):
    if np.asarray(got).dtype != np.asarray(want).dtype:
        return name, 'FAIL dtype %s, reference %s' % (np.asarray(got).dtype, np.asarray(want).dtype)
    return name, 'ok' if close(got, want, rtol, atol) else 'FAIL values'


def ref_humidity(rng):
    from oracle import pgw_oracle_refdtype as R
    shp = (int(rng.integers(1, 3)), int(rng.integers(1, 12)), int(rng.integers(1, 6)), int(rng.integers(1, 9)))
    a, b, c = _dt(rng), _dt(rng), _dt(rng)
    ta = rng.uniform(185.0, 320.0, shp).astype(c)
    pa = rng.uniform(1.0e3, 1.05e5, shp).astype(b)
    which = int(rng.integers(0, 5))
    tol = 1e-12 if c == np.float64 else EXP_F32
    if which == 0:
        hus = (10.0 ** rng.uniform(-7, -1.7, shp)).astype(a)
        got, want, note = both(lambda: F.specific_to_relative_humidity(hus, pa, ta), lambda: R.specific_to_relative_humidity(hus, pa, ta))
    elif which == 1:
        hur = rng.uniform(0.5, 120.0, shp).astype(a)
        got, want, note = both(lambda: F.relative_to_specific_humidity(hur, pa, ta), lambda: R.relative_to_specific_humidity(hur, pa, ta))
    elif which == 2:
        hus = (10.0 ** rng.uniform(-7, -1.7, shp)).astype(a)
        got, want, note = both(lambda: F.specific_humidity_to_vapor_pressure(hus, pa), lambda: R.specific_humidity_to_vapor_pressure(hus, pa))
        tol = 0.0
    elif which == 3:
        e = rng.uniform(0.0, 900.0, shp).astype(a)
        got, want, note = both(lambda: F.vapor_pressure_to_specific_humidity(e, pa), lambda: R.vapor_pressure_to_specific_humidity(e, pa))
        tol = 0.0
    else:
        got, want, note = both(lambda: F.saturation_vapor_pressure_water_and_ice(pa, ta), lambda: R.saturation_vapor_pressure_water_and_ice(pa, ta))
    return ('ref_humidity_%d' % which, note) if note else _verdict('ref_humidity_%d' % which, got, want, tol)


def ref_geopot(rng):
    from oracle import pgw_oracle_refdtype as R
    nlat, nlon, nlev, seed = int(rng.integers(1, 7)), int(rng.integers(1, 9)), int(rng.integers(6, 40)), int(rng.integers(0, 1 << 30))
    era = synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=seed, dtype=np.float32)['era']
    pa_hl = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])[0]
    z, t, q = era['FIS'].astype(_dt(rng)), era['T'].astype(_dt(rng)), era['QV'].astype(_dt(rng))
    level1 = np.arange(1, nlev + 2)
    r = rng.random()
    p_ref = float(rng.choice([30000.0, 50000.0, 20000.0])) if r < 0.5 else (
        rng.uniform(1.0e4, 0.9 * era['PS'].min(), era['PS'].shape) if r < 0.9 else 2.0e5)
    got, want, note = both(lambda: F.integ_geopot(pa_hl, z, t, q, level1, p_ref), lambda: R.integ_geopot(pa_hl, z, t, q, level1, p_ref))
    if note:
        return 'ref_integ_geopot', note
    if got.dtype != want.dtype:
        return 'ref_integ_geopot', 'FAIL dtype %s' % got.dtype
    ulp = np.spacing(np.abs(want).astype(np.float32 if z.dtype == np.float32 else np.float64)).astype(np.float64)
    return 'ref_integ_geopot', 'ok' if np.all(np.abs(got - want) <= np.maximum(ulp, 1e-11 * np.abs(want))) else 'FAIL values'


def ref_interp(rng):
    from oracle import pgw_oracle_refdtype as R
    nt, S, N, nlat, nlon = int(rng.integers(1, 3)), int(rng.integers(2, 24)), int(rng.integers(1, 50)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
    sp = np.sort(rng.uniform(50., 1.05e5, (nt, S, nlat, nlon)), axis=1)
    tp = np.sort(rng.uniform(20., 1.09e5, (nt, N, nlat, nlon)), axis=1)
    var = rng.normal(size=(nt, S, nlat, nlon)).astype(_dt(rng))
    mode = str(rng.choice(['off', 'linear', 'constant', 'nan']))
    if mode == 'off' and rng.random() < 0.8:
        tp = np.clip(tp, sp[:, :1], sp[:, -1:])
    got, want, note = both(lambda: F.interp_logp_4d(var, sp, tp, mode), lambda: R.interp_logp_4d(var, sp, tp, mode))
    return ('ref_interp_' + mode, note) if note else _verdict('ref_interp_' + mode, got, want, 1e-9, 1e-9)


def ref_vert(rng):
    from oracle import pgw_oracle_refdtype as R
    nlat, nlon, N = int(rng.integers(1, 6)), int(rng.integers(1, 9)), int(rng.integers(2, 40))
    plev = synthetic.PLEV19
    delta = rng.normal(size=(1, len(plev), nlat, nlon)).astype(_dt(rng))
    tp = np.sort(rng.uniform(120., 1.06e5, (1, N, nlat, nlon)), axis=1)
    with_sfc = rng.random() < 0.6
    dsfc = rng.normal(size=(1, nlat, nlon)).astype(_dt(rng)) if with_sfc else None
    psh = rng.uniform(4.0e4, 1.06e5, (1, nlat, nlon)).astype(_dt(rng)) if with_sfc else None
    if with_sfc and rng.random() < 0.1:
        psh[0, 0, 0] = 50.0
    got, want, note = both(lambda: F.vert_interp_delta(delta, tp, dsfc, psh, True, plev=plev),
                           lambda: R.vert_interp_delta(delta, plev, tp, dsfc, psh, True))
    return ('ref_vert_interp_delta', note) if note else _verdict('ref_vert_interp_delta', got, want, 1e-9, 1e-9)


def ref_riders(rng):
    from oracle import pgw_oracle_refdtype as R
    shp = (int(rng.integers(1, 9)), int(rng.integers(1, 12)))
    if rng.random() < 0.5:
        vb, va = rng.normal(size=shp).astype(_dt(rng)), rng.normal(size=shp).astype(_dt(rng))
        x_hi = float(np.timedelta64(31, 'D').astype('timedelta64[ns]').astype(np.int64))
        x_new = float(np.timedelta64(int(rng.integers(1, 31)), 'D').astype('timedelta64[ns]').astype(np.int64))
        t1 = np.datetime64('2006-01-01') + np.timedelta64(int(x_new), 'ns')
        got, want, note = both(lambda: F.time_lerp(vb, va, x_hi, x_new), lambda: R.time_lerp(vb, va, '2006-01-01', '2006-02-01', t1))
        return ('ref_time_lerp', note) if note else _verdict('ref_time_lerp', got, want, 0.0)
    tos = rng.normal(1.5, 0.5, shp); tos[rng.uniform(size=shp) < 0.3] = np.nan
    ice = np.clip(rng.uniform(-0.5, 1.0, shp), 0, 1); ice[rng.uniform(size=shp) < 0.25] = np.nan
    ops = [x.astype(_dt(rng)) for x in (tos, rng.normal(2.5, 0.5, shp), np.clip(rng.uniform(-0.3, 1.3, shp), 0, 1), ice)]
    got, want, note = both(lambda: F.integrate_tos(*ops), lambda: R.integrate_tos(*ops))
    return ('ref_integrate_tos', note) if note else _verdict('ref_integrate_tos', got, want, 0.0)


REF_CASES = [ref_humidity, ref_humidity, ref_geopot, ref_interp, ref_interp, ref_vert, ref_vert, ref_riders]

CASES = [case_interp, case_interp, case_vert, case_vert, case_geopot, case_humidity, case_regrid, case_regrid, case_smooth,
         case_ocean]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--cases', type=int, default=400)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--dtype-flow', choices=['common', 'reference'], default='common',
                   help="'reference': random dtype mixes under settings.function_dtype_flow = 'reference' against the reference-dtype oracle")
    a = p.parse_args()
    cases = CASES
    if a.dtype_flow == 'reference':
        from pgw4era5_amd import settings
        settings.function_dtype_flow = 'reference'
        cases = REF_CASES
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    counts, fails = {}, []
    for i in range(a.cases):
        fn = cases[int(rng.integers(0, len(cases)))]
        state = rng.bit_generator.state
        name, res = fn(rng)
        key = res if res in ('ok', 'both raise') else 'FAIL'
        counts[name + ':' + key] = counts.get(name + ':' + key, 0) + 1
        if key == 'FAIL':
            fails.append(dict(i=i, case=name, result=res[:300]))
            print(json.dumps(fails[-1]), flush=True)
        del state
    print(json.dumps(dict(cases=a.cases, seed=a.seed, **({'dtype_flow': 'reference'} if a.dtype_flow == 'reference' else {}), seconds=round(time.time() - t0, 1), counts=dict(sorted(counts.items())),
                         failures=fails[:20])))
    return 1 if fails else 0


if __name__ == '__main__':
    sys.exit(main())
