"""settings.function_dtype_flow = 'reference', the part that needs no GPU:
(1) `functions.reference_dtype_flow` - the helper that turns operand dtypes into C-ABI tags and the result dtype - gives,
    for every function and every float32 / float64 mix the flow allows, the dtype oracle/pgw_oracle_refdtype.py returns on
    tiny arrays of those dtypes; a float32 pressure raises NotImplementedError; a bad setting raises ValueError;
(2) the rehearsal loop of tests/dtype_flow_rehearsal.py, run with the reference-dtype oracle's functions, gives that
    oracle's own whole-file n_iter, max_err and PS bit for bit - so the GPU rehearsal measures the functions, not the loop."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtype_flow_rehearsal as DR                                                    # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402
from pgw4era5_amd import _lib, functions as F, settings                              # noqa: E402

f4, f8 = np.dtype('float32'), np.dtype('float64')
TAG = {f4: _lib.PGW_F32, f8: _lib.PGW_F64}


def mixes(n):
    return list(itertools.product((f4, f8), repeat=n))


def check(function, want, **dts):
    tags, res = F.reference_dtype_flow(function, **dts)
    assert tags == {k: TAG[np.dtype(v)] for k, v in dts.items() if v is not None}, (function, dts)
    if isinstance(want, tuple):
        assert tuple(np.dtype(r) for r in res) == tuple(w.dtype for w in want), (function, dts)
    else:
        assert np.dtype(res) == want.dtype, (function, dts, res, want.dtype)


def test_helper_humidity_result_dtypes():
    hus, pa, ta = np.array([3e-3, 1e-4]), np.array([9e4, 4e4]), np.array([285.0, 255.0])
    for a, b in mixes(2):
        check('specific_humidity_to_vapor_pressure', R.specific_humidity_to_vapor_pressure(hus.astype(a), pa.astype(b)), hus=a, pa=b)
        check('vapor_pressure_to_specific_humidity', R.vapor_pressure_to_specific_humidity((hus * 1e5).astype(a), pa.astype(b)), vapp=a, pa=b)
    for (t,) in mixes(1):
        for water in (True, False):
            check('saturation_vapor_pressure_water_or_ice', R.saturation_vapor_pressure_water_or_ice(pa, ta.astype(t), water), ta=t)
        check('saturation_vapor_pressure_water_and_ice', R.saturation_vapor_pressure_water_and_ice(pa, ta.astype(t)), ta=t)
    for a, b, c in mixes(3):
        check('specific_to_relative_humidity', R.specific_to_relative_humidity(hus.astype(a), pa.astype(b), ta.astype(c)), hus=a, pa=b, ta=c)
        check('relative_to_specific_humidity', R.relative_to_specific_humidity((hus * 1e4).astype(a), pa.astype(b), ta.astype(c)),
              hur=a, pa=b, ta=c)
    # the mix a float32 file produces
    assert F.reference_dtype_flow('specific_to_relative_humidity', hus=f4, pa=f8, ta=f4)[1] == f8


def test_helper_integ_geopot_and_interpolation_result_dtypes():
    c = DR.f32_case((3, 4, 8), 7)
    era = c['era']
    pa_hl, pa = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    assert pa_hl.dtype == f8
    lvl = np.arange(1, 10)
    for z, t, q in mixes(3):
        want = R.integ_geopot(pa_hl, era['FIS'].astype(z), era['T'].astype(t), era['QV'].astype(q), lvl, 30000.0)
        check('integ_geopot', want, pa_hl=f8, zgs=z, ta=t, hus=q)
        check('integ_geopot', want, pa_hl=f8, zgs=z, ta=t, hus=q, p_ref=f8)
        assert F.reference_dtype_flow('integ_geopot', pa_hl=f8, zgs=z, ta=t, hus=q, p_ref=None)[1] == f8
    src = np.sort(np.random.default_rng(0).uniform(1e3, 1e5, (1, 5, 2, 2)), axis=1)
    trg = np.sort(np.random.default_rng(1).uniform(1e3, 1e5, (1, 4, 2, 2)), axis=1)
    for (v,) in mixes(1):
        var = np.random.default_rng(2).normal(size=src.shape).astype(v)
        for mode in ('linear', 'constant', 'nan'):
            want = R.interp_logp_4d(var, src, trg, mode)
            check('interp_logp_4d', want, var=v, source_P=f8, targ_P=f8)
            check('interp_1d_for_timelatlon', want, orig_array=v, src_p=f8, targ_p=f8)
            check('interp_extrap_1d', want, src_y=v, src_x=f8, targ_x=f8)
    plev = np.array([1e5, 7e4, 3e4, 1e4, 2e3])
    for d, s, h in mixes(3):
        delta = np.random.default_rng(3).normal(size=(1, 5, 2, 2)).astype(d)
        dsfc = np.ones((1, 2, 2), s); psh = np.full((1, 2, 2), 9.5e4, h)
        want = R.vert_interp_delta(delta, plev, trg, dsfc, psh, True)
        for a in (f4, f8, None):
            check('vert_interp_delta', want, delta=d, delta_sfc=s, ps_hist=h, target_P=f8, add_to=a)
        check('vert_interp_delta', R.vert_interp_delta(delta, plev, trg, None, None, True), delta=d, target_P=f8)
        # replace_delta_sfc: P float64, D in the delta's dtype (tests/golden/ref_leaf_f32_vectors.npz: rds_out_P, rds_out_D)
        check('replace_delta_sfc', (np.zeros(1, f8), np.zeros(1, d)), source_P=f8, delta=d, delta_sfc=s, ps_hist=h)


def test_helper_time_lerp_and_integrate_tos_result_dtypes():
    for b, a in mixes(2):
        want = R.time_lerp(np.ones(3, b), np.full(3, 2.5, a), '2006-01-01', '2006-02-01', '2006-01-11')
        check('time_lerp', want, v_before=b, v_after=a)
    for m in mixes(4):
        arrs = [np.array([[0.3, 0.6]], d) for d in m]
        check('integrate_tos', R.integrate_tos(*arrs), **dict(zip(('tos_field', 'ts_field', 'land_frac', 'ice_frac'), m)))


@pytest.mark.parametrize('function,bad', [('integ_geopot', 'pa_hl'), ('integ_geopot', 'p_ref'), ('interp_logp_4d', 'source_P'),
                                          ('interp_logp_4d', 'targ_P'), ('interp_1d_for_timelatlon', 'src_p'),
                                          ('interp_1d_for_timelatlon', 'targ_p'), ('interp_extrap_1d', 'src_x'),
                                          ('interp_extrap_1d', 'targ_x'), ('vert_interp_delta', 'target_P'),
                                          ('replace_delta_sfc', 'source_P')])
def test_float32_pressure_is_not_computed_in_float64_under_the_name_reference(function, bad):
    with pytest.raises(NotImplementedError) as e:
        F.reference_dtype_flow(function, **{bad: f4})
    assert bad in str(e.value) and "'common'" in str(e.value)
    F.reference_dtype_flow(function, **{bad: f8})


def test_bad_setting_value_and_default(monkeypatch):
    assert settings.function_dtype_flow == 'common'
    monkeypatch.setattr(settings, 'function_dtype_flow', 'fast')
    with pytest.raises(ValueError) as e:
        F._flow()
    assert 'function_dtype_flow' in str(e.value)
    monkeypatch.setattr(settings, 'function_dtype_flow', 'reference')
    assert F._flow() == 'reference'
    with pytest.raises(ValueError):
        F.reference_dtype_flow('hybrid_pressure', ps=f4)


@pytest.mark.parametrize('shape,seed', DR.SHAPES)
def test_rehearsal_with_the_oracle_functions_is_the_oracle_loop(shape, seed):
    c = DR.f32_case(shape, seed)
    run, ta_pgw, hur_pgw, dzg = DR.oracle_file_run(c)
    got = DR.rehearsal(R.relative_to_specific_humidity, R.integ_geopot, c['era'], ta_pgw, hur_pgw, dzg)
    assert got['n_iter'] == run['n_iter']
    assert got['max_err'] == run['max_err']
    assert got['PS'].dtype == run['PS'].dtype == np.float32
    np.testing.assert_array_equal(got['PS'], run['PS'])
    # and the same loop on float64 copies through the float64 oracle (today's function-level flow) is NOT that loop
    # (PS stays float32 in the script - the file's array; only the functions see float64 copies)
    common = DR.rehearsal(lambda h, p, t: O.relative_to_specific_humidity(np.float64(h), np.float64(p), np.float64(t)),
                          lambda p, z, t, q, l, pr: O.integ_geopot(np.float64(p), np.float64(z), np.float64(t), np.float64(q), l, pr),
                          c['era'], ta_pgw, hur_pgw, dzg)
    n = min(len(common['max_err']), len(run['max_err']))
    assert np.max(np.abs(np.array(common['max_err'][:n]) - np.array(run['max_err'][:n]))) > 2e-3
