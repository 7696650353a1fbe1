"""CPU tests of the edge inputs the surface-rider GPU tests run on (tests/surface_edge_cases.py): every named edge is
really in the built arrays, in float64 and after the cast to float32; the float64 oracle puts its NaNs exactly where the
construction predicts; the reference-dtype oracle is the float64 oracle on float64 operands."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_edge_cases as E                                                       # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

DTYPES = ('float64', 'float32')


def _ice(inp, c, t=0):
    """sic + dsic / 100 before the clip, in float64 on the stored values (what every mode but the reference one takes)."""
    return np.float64(inp.sic[t, c]) + np.float64(inp.dsic[t, c]) / 100


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_named_edge_is_in_the_built_inputs(dtype):
    inp = E.build(300, dtype, nsoil=16, ntime=3)
    T = inp.dtype.type
    assert inp.names == E.NAMES and inp.sic.dtype == inp.dtos.dtype == inp.land.dtype == inp.tso.dtype == inp.dtype
    assert inp.sic.shape == inp.dsic.shape == inp.dtos.shape == inp.dts.shape == inp.tskin.shape == (3, 300)
    assert inp.land.shape == inp.clim.shape == (300,) and inp.tso.shape == (3, 16, 300)
    nan = np.isnan
    sic, dsic, tos, ts, land = inp.sic[0], inp.dsic[0], inp.dtos[0], inp.dts[0], inp.land
    c = lambda name: E.col(inp, name)
    # ---- the mask disagreements
    k = c('sic_nan_tos_finite'); assert nan(sic[k]) and not nan(tos[k]) and not nan(dsic[k])
    k = c('sic_finite_tos_nan'); assert not nan(sic[k]) and not nan(dsic[k]) and nan(tos[k])
    k = c('dsic_nan_sic_finite'); assert nan(dsic[k]) and not nan(sic[k]) and not nan(tos[k])
    k = c('both_nan'); assert nan(sic[k]) and nan(tos[k])
    k = c('land_nan_in_mask'); assert nan(land[k]) and not (nan(sic[k]) or nan(dsic[k]) or nan(tos[k]) or nan(ts[k]))
    k = c('land_nan_out_mask'); assert nan(land[k]) and nan(sic[k]) and not nan(ts[k])
    k = c('ts_nan_in_mask'); assert nan(ts[k]) and not (nan(sic[k]) or nan(dsic[k]) or nan(tos[k]) or nan(land[k]))
    k = c('ts_nan_out_mask'); assert nan(ts[k]) and nan(sic[k])
    # ---- the ice update at its clip: exact ties stay exact in float64 arithmetic on the stored values AND in float32
    # arithmetic (reference mode on an exact record), whatever the storage dtype
    f4 = np.float32
    ice32 = lambda k: f4(sic[k]) + f4(dsic[k]) / f4(100)
    for name, want in (('ice_exact_0', 0.0), ('ice_exact_1', 1.0), ('frac_exact_0', 0.0), ('pure_tos', 0.0)):
        assert _ice(inp, c(name)) == want and ice32(c(name)) == want, name
    assert _ice(inp, c('ice_ulp_above_0')) == np.nextafter(T(0), T(1)) > 0
    assert _ice(inp, c('ice_ulp_below_0')) == -np.nextafter(T(0), T(1)) < 0
    assert _ice(inp, c('ice_ulp_below_1')) == np.nextafter(T(1), T(0)) < 1
    assert _ice(inp, c('ice_ulp_above_1')) == np.nextafter(T(1), T(2)) > 1
    assert _ice(inp, c('ice_far_below_0')) < -0.5 and _ice(inp, c('ice_far_above_1')) > 1.5
    k = c('dsic_neg_zero'); assert dsic[k] == 0 and np.signbit(dsic[k])
    # ---- the blend fraction at its clip
    ice = np.clip(np.array([_ice(inp, k) for k in range(inp.ntable)]), 0, 1)
    k = c('frac_exact_1'); assert ice[k] + np.float64(land[k]) == 1.0 and 0 < ice[k] < 1 and f4(ice[k]) + f4(land[k]) == 1
    k = c('frac_exact_0'); assert ice[k] + np.float64(land[k]) == 0.0
    k = c('frac_above_1'); assert land[k] == 1 and ice[k] > 0
    k = c('pure_tos'); assert land[k] == 0 and ice[k] == 0
    k = c('pure_ts'); assert land[k] == 1
    # ---- float32 cancellation: float32 numbers in either storage, and the float32 sum is not the rounded float64 sum
    for name, d in (('cancel_below', np.nextafter(f4(-20), f4(-np.inf))), ('cancel_above', np.nextafter(f4(-20), f4(0)))):
        k = c(name)
        assert sic[k] == f4(0.2) and dsic[k] == d
        assert ice32(k) != f4(_ice(inp, k)), name                     # order-sensitive: the two flows part here
        assert (ice32(k) < 0) == (_ice(inp, k) < 0)
    # ---- soil depths
    assert list(E.soil_depths(4)) == list(E.ERA_DEPTHS) and list(E.soil_depths(1)) == [0.0]
    z = E.soil_depths(16)
    assert len(z) == 16 and z[0] == 0.0 and np.exp(-z[0] / 2.8) == 1.0 and np.exp(-z[-1] / 2.8) == 0.0
    assert set(E.ERA_DEPTHS) <= set(z)
    # ---- no two neighbouring columns alike, no two time steps alike (a wrong index or slab shows)
    assert np.all(ts[:-1][~nan(ts[:-1])] != ts[1:][~nan(ts[:-1])])
    assert np.all(inp.tskin[:, :-1] != inp.tskin[:, 1:]) and np.all(inp.tso[..., :-1] != inp.tso[..., 1:])
    for t in (1, 2):
        for x in (inp.sic, inp.dsic, inp.dtos, inp.dts):
            assert not np.array_equal(x[t], x[0], equal_nan=True) and not np.array_equal(x[t], x[t - 1], equal_nan=True)
        assert np.isnan(inp.sic[t]).sum() == np.isnan(inp.sic[0]).sum()
    # the float32 build holds the float64 build's numbers, except the storage-ulp columns
    if dtype == 'float32':
        big = E.build(300, 'float64', nsoil=16, ntime=3)
        ulp = [c(n) for n in E.NAMES if '_ulp_' in n]
        for a, b in ((inp.sic, big.sic), (inp.dsic, big.dsic), (inp.dtos, big.dtos), (inp.dts, big.dts)):
            keep = np.setdiff1d(np.arange(inp.ntable), ulp)
            np.testing.assert_array_equal(a[0, keep].astype(np.float64), b[0, keep])          # the table: no rounding at all
            keep = np.setdiff1d(np.arange(300), ulp)
            np.testing.assert_array_equal(a[0, keep], b[0, keep].astype(np.float32))


@pytest.mark.parametrize('ncol', E.NCOLS)
def test_column_counts(ncol):
    inp = E.build(ncol, 'float64')
    assert inp.sic.shape == (1, ncol) and inp.ntable == min(ncol, len(E.NAMES))
    assert inp.names == E.NAMES[:ncol]


@pytest.mark.parametrize('ntime', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_oracle_nans_are_exactly_the_predicted_ones(dtype, ntime):
    """O.sea_ice_update, O.integrate_tos and O.soil_temperature_delta on the edge inputs: NaN in the predicted columns and
    nowhere else; the table's own expectations (clipped to 0 / 1, pure ts, pure tos) hold in time step 0."""
    for ncol in E.NCOLS:
        for nsoil in E.NSOILS:
            inp = E.build(ncol, dtype, nsoil=nsoil, ntime=ntime)
            want = E.oracle_update(inp)
            np.testing.assert_array_equal(np.isnan(want['sic']), inp.nan_ice)
            np.testing.assert_array_equal(np.isnan(want['comb']), inp.nan_comb)
            np.testing.assert_array_equal(np.isnan(want['dsoil']), inp.nan_soil)
            np.testing.assert_array_equal(np.isnan(want['tskin']), inp.nan_comb)
            np.testing.assert_array_equal(np.isnan(want['tso']), inp.nan_soil)
            assert want['tso'].shape == (ntime, nsoil, ncol)
            for c, (name, ik, ck) in enumerate(zip(inp.names, inp.ice_kind, inp.comb_kind)):
                ice, comb = want['sic'][0, c], want['comb'][0, c]
                ok = dict(nan=np.isnan(ice), zero=ice == 0, one=ice == 1, open=0 < ice < 1)[ik]
                assert ok, (name, ik, ice)
                ok = dict(nan=np.isnan(comb), ts=comb == inp.dts[0, c], tos=comb == inp.dtos[0, c], finite=np.isfinite(comb))[ck]
                assert ok, (name, ck, comb)
            if nsoil == 16:                       # w = 1 at the surface: the whole delta; w = 0 at depth: the climatology
                ok = ~inp.nan_comb
                np.testing.assert_array_equal(want['dsoil'][:, 0][ok], (E.f64(inp.clim)[None] + (want['comb'] - E.f64(inp.clim)[None]))[ok])
                np.testing.assert_array_equal(want['dsoil'][:, 15][ok], np.broadcast_to(E.f64(inp.clim)[None], ok.shape)[ok])
    assert inp.nan_comb.any() and not inp.nan_comb.all() and inp.nan_ice.any()


def test_refdtype_oracle_is_the_float64_oracle_on_float64_operands():
    """R.integrate_tos == O.integrate_tos bit for bit when every operand is float64 (the reference flow has nothing to
    promote), on the edge table and with the ice of time step 0 at every step."""
    for ntime in (1, 3):
        inp = E.build(300, 'float64', ntime=ntime)
        ice = O.sea_ice_update(inp.sic, inp.dsic)
        args = (inp.dtos, inp.dts, np.broadcast_to(inp.land[None], inp.dtos.shape), np.broadcast_to(ice[0][None], inp.dtos.shape))
        a, b = R.integrate_tos(*args), O.integrate_tos(*args)
        assert a.dtype == b.dtype == np.float64
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(np.signbit(a), np.signbit(b))
        np.testing.assert_array_equal(np.isnan(a), inp.nan_comb)


@pytest.mark.parametrize('mode', E.MODES)
def test_delta_records_keep_the_edges_through_the_time_interpolation(mode):
    """The records the GPU tests hand to a DeltaSet: the table columns are equal in all records, so load_delta_values
    returns them exactly at an interpolated instant too; on per-variable time axes exactly the chosen variables hit a record."""
    import datetime as dt
    dtype = E.DTYPE[mode]
    inp = E.build(300, dtype)
    ora = R if mode == 'f32_reference' else O
    target = dt.datetime(2006, 8, 2, 3)
    for on in ((), ('siconc',), ('tos', 'ts'), ('siconc', 'tos', 'ts')):
        c = E.mixed_axis_case(inp, on, target)
        for var, base in (('siconc', inp.dsic), ('tos', inp.dtos), ('ts', inp.dts)):
            src = c['deltas'][var] if ora is R else E.f64(c['deltas'][var])
            got = ora.load_delta_values(src, c['delta_times'][var], target)
            assert got.shape == (1, 1, 300)
            np.testing.assert_array_equal(got[0, 0, :inp.ntable], E.f64(base[0, :inp.ntable]))
            if ora is R:
                assert got.dtype == (np.float32 if var in on else np.float64), (var, on)
            if var in on:
                np.testing.assert_array_equal(got[0], c['deltas'][var][7])
            else:
                assert not np.array_equal(got[0], c['deltas'][var][6], equal_nan=True)
        comb, dsoil = E.oracle_surface_deltas(c, mode, np.zeros((1, 300)))
        assert comb.shape == (1, 1, 300) and dsoil.shape == (1, 4, 1, 300) and comb.dtype == np.float64
