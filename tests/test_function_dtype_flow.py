"""settings.function_dtype_flow = 'reference' on the GPU: the function-level API follows the reference's dtype flow -
every operand in its own dtype, numpy's promotion reproduced by the kernels (`pgw_*_mixed` of include/pgw_hip.h), the result
in the dtype the reference returns.  What the reference computes is defined by oracle/pgw_oracle_refdtype.py and by
tests/golden/ref_leaf_f32_vectors.npz (written by the reference's own leaf functions).

Bounds.  float32 operations are single IEEE operations on the device, so everything that is arithmetic only is asserted bit
for bit.  Not numpy's last bit: device expf (4 float32 ulp, the bound test_reference_mode_esat_f32_fast_path_is_the_literal_
expression holds it to) and the fp64 logarithm (<= 1 ulp, test_device_log_accuracy).  In integ_geopot a last-bit change of
ln p can turn a float32 rounding of phi_hl the other way with a probability of the order 1e-8 per level: every column within
one float32 ulp of |phi|, at least 99 % of the columns bit-identical (the float64 flow has 0 % and exceeds one ulp)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtype_flow_rehearsal as DR                                                    # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
f4, f8 = np.float32, np.float64
ULP4_F32 = 4 * 2.0 ** -23


@pytest.fixture(scope='module')
def F():
    from pgw4era5_amd import functions
    return functions


@pytest.fixture
def ref_flow(monkeypatch):
    from pgw4era5_amd import settings
    monkeypatch.setattr(settings, 'function_dtype_flow', 'reference')
    return settings


@pytest.fixture(scope='module')
def g32():
    return dict(np.load(os.path.join(GOLDEN, 'ref_leaf_f32_vectors.npz'), allow_pickle=False))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype, (a.dtype, b.dtype)
    np.testing.assert_array_equal(a, b)


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------ 3: golden leaves of the reference
def test_golden_leaves_bit_for_bit_and_in_the_stored_dtype(F, ref_flow, g32):
    g = g32
    same(F.specific_humidity_to_vapor_pressure(g['hum_hus'], g['hum_pa']), g['hum_e'])
    same(F.specific_humidity_to_vapor_pressure(g['hum_hus'], g['hum_pa'].astype(f4)), g['hum_e_allf32'])
    same(F.vapor_pressure_to_specific_humidity(g['hum_e'], g['hum_pa']), g['hum_q_from_e'])
    for mode in ('constant', 'linear'):
        got = np.stack([F.interp_extrap_1d(g['int_src_x'][c], g['int_src_y'][c], g['int_targ_x'][c], mode)
                        for c in range(g['int_src_x'].shape[0])])
        same(got, g['int_' + mode])
    for i, ps in enumerate(g['rds_ps']):
        P, D = F.replace_delta_sfc(g['rds_plev'], ps, g['rds_delta'], np.float32(9.25))
        same(P, g['rds_out_P'][i])
        same(D, g['rds_out_D'][i])
    same(F.integrate_tos(g['tos_tos'], g['tos_ts'], g['tos_land'], g['tos_ice']), g['tos_out'])
    same(F.integrate_tos(g['tos_tos'].astype(f4), g['tos_ts'].astype(f4), g['tos_land'], g['tos_ice']), g['tos_out_allf32'])
    for water, key in ((True, 'hum_esat_water'), (False, 'hum_esat_ice')):
        got = F.saturation_vapor_pressure_water_or_ice(g['hum_pa'], g['hum_ta'], water=water)
        assert got.dtype == np.float32
        print(key, 'max rel', np.max(np.abs(f64(got) - f64(g[key])) / f64(g[key])))
        np.testing.assert_allclose(f64(got), f64(g[key]), rtol=ULP4_F32, atol=0)


# ------------------------------------------------------------------ 4: integ_geopot
def _geopot_check(got, want):
    assert got.dtype == np.float64 and want.dtype == np.float64
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = np.max(np.abs(got - want) / ulp)
    identical = np.mean(got == want)
    print('   worst %.3f float32 ulp of |phi|, %.2f %% of the columns bit-identical' % (worst, 100 * identical))
    assert worst <= 1.0
    assert identical >= 0.99


@pytest.mark.parametrize('full', [True, False])
@pytest.mark.parametrize('shape,seed', DR.SHAPES)
def test_integ_geopot_reference_flow(F, ref_flow, shape, seed, full):
    era = DR.f32_case(shape, seed)['era']
    pa_hl, _ = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    assert pa_hl.dtype == np.float64
    lvl = np.arange(1, shape[2] + 2)
    FIS, T, QV = era['FIS'], era['T'], era['QV']
    pf = np.where(era['PS'] > 90000, 50000.0, 30000.0)
    for p_ref in (30000.0, pf):
        _geopot_check(F.integ_geopot(pa_hl, FIS, T, QV, lvl, p_ref, full_column=full), R.integ_geopot(pa_hl, FIS, T, QV, lvl, p_ref))
    # the float64 flow on the same values is not that: no column identical, more than one ulp away (on the CPU)
    want = R.integ_geopot(pa_hl, FIS, T, QV, lvl, 30000.0)
    c64 = O.integ_geopot(pa_hl, f64(FIS), f64(T), f64(QV), lvl, 30000.0)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.mean(c64 == want) < 0.5 and np.max(np.abs(c64 - want) / ulp) > 1.0
    # mixes: zgs float64 beside a float32 state; zgs float32 beside the float64 PGW state of the loop; ta float32, hus float64
    T64 = f64(T) + 1.25
    for z, t, q in ((FIS, T64, f64(QV) * 1.01), (FIS, T, f64(QV) * 1.01), (FIS, T64, QV)):
        _geopot_check(F.integ_geopot(pa_hl, z, t, q, lvl, 30000.0, full_column=full), R.integ_geopot(pa_hl, z, t, q, lvl, 30000.0))
    # a float64 zgs: phi_hl is float64, no rounding absorbs the last bit of the logarithm - the bound of the float64 function
    # against its oracle (test_integ_geopot_vs_oracle: 1e-9), 50 times below one float32 ulp; tav is float32 for a float32
    # state, which float64 arithmetic on the same values misses by more than that
    for t, q in ((T, QV), (f64(T), QV), (T, f64(QV))):
        got, want = F.integ_geopot(pa_hl, f64(FIS), t, q, lvl, 30000.0, full_column=full), R.integ_geopot(pa_hl, f64(FIS), t, q, lvl, 30000.0)
        assert got.dtype == want.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    c64 = O.integ_geopot(pa_hl, f64(FIS), f64(T), f64(QV), lvl, 30000.0)
    assert not np.allclose(c64, R.integ_geopot(pa_hl, f64(FIS), T, QV, lvl, 30000.0), rtol=1e-9, atol=0)


def test_integ_geopot_reference_flow_errors_on_float32_operands(F, ref_flow):
    """The three error cases of test_integ_geopot_isothermal_exact_and_errors, float32 zgs / ta / hus."""
    from pgw4era5_amd import synthetic
    era = synthetic.make_case(nlat=6, nlon=8, nlev=30, seed=5, dtype=np.float32)['era']
    pa_hl, pa = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    T = np.full(pa.shape, 250.0, f4); q = np.zeros(pa.shape, f4)
    lvl = np.arange(1, 32)
    _geopot_check(F.integ_geopot(pa_hl, era['FIS'], T, q, lvl, 30000.0), R.integ_geopot(pa_hl, era['FIS'], T, q, lvl, 30000.0))
    with pytest.raises(ValueError) as e:
        F.integ_geopot(pa_hl, era['FIS'], T, q, lvl, 200000.0)
    assert 'p_ref locally lies below the surface' in str(e.value)
    with pytest.raises(KeyError):
        F.integ_geopot(pa_hl, era['FIS'], T, q, lvl, 1e-5)
    p2 = pa_hl.copy(); p2[0, 10, 2, 3] = 95000.0           # non-monotone column: the reference's nanargmin rule
    _geopot_check(F.integ_geopot(p2, era['FIS'], T, q, lvl, 30000.0), R.integ_geopot(p2, era['FIS'], T, q, lvl, 30000.0))
    with pytest.raises(NotImplementedError) as e:          # a float32 pressure is not computed in float64 under this name
        F.integ_geopot(pa_hl.astype(f4), era['FIS'], T, q, lvl, 30000.0)
    assert 'pa_hl' in str(e.value)


# ------------------------------------------------------------------ 5: the other functions
@pytest.mark.parametrize('shape,seed', DR.SHAPES)
def test_humidity_pair_all_mixes(F, ref_flow, shape, seed):
    era = DR.f32_case(shape, seed)['era']
    _, pa = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    rh64 = R.specific_to_relative_humidity(f64(era['QV']), pa, f64(era['T']))
    for a in (f4, f8):
        for b in (f4, f8):
            for c in (f4, f8):
                tol = 1e-12 if c == f8 else ULP4_F32
                q, p, t = era['QV'].astype(a), pa.astype(b), era['T'].astype(c)
                got, want = F.specific_to_relative_humidity(q, p, t), R.specific_to_relative_humidity(q, p, t)
                assert got.dtype == want.dtype, (a, b, c)
                print('q->RH', a.__name__, b.__name__, c.__name__, 'max rel %.3e' % np.max(np.abs(f64(got) - f64(want)) / np.abs(f64(want))))
                np.testing.assert_allclose(f64(got), f64(want), rtol=tol, atol=0)
                h = rh64.astype(a)
                got, want = F.relative_to_specific_humidity(h, p, t), R.relative_to_specific_humidity(h, p, t)
                assert got.dtype == want.dtype, (a, b, c)
                print('RH->q', a.__name__, b.__name__, c.__name__, 'max rel %.3e' % np.max(np.abs(f64(got) - f64(want)) / np.abs(f64(want))))
                np.testing.assert_allclose(f64(got), f64(want), rtol=tol, atol=0)
    # mixed-phase e_sat leaf in the dtype of ta
    got = F.saturation_vapor_pressure_water_and_ice(pa, era['T'])
    assert got.dtype == np.float32
    np.testing.assert_allclose(f64(got), f64(R.saturation_vapor_pressure_water_and_ice(pa, era['T'])), rtol=ULP4_F32)


def _interp_inputs(shape, seed, mode):
    era = DR.f32_case(shape, seed)['era']
    _, src = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    if mode == 'off':
        trg = 0.5 * (src[:, 1:] + src[:, :-1])
    else:
        _, trg = R.hybrid_pressure(era['ak'], era['bk'], era['PS'] + np.float32(900.0))
    return era['U'], src, trg


@pytest.mark.parametrize('mode', ['off', 'linear', 'constant', 'nan'])
@pytest.mark.parametrize('shape,seed', DR.SHAPES)
def test_interp_logp_4d_float32_var(F, shape, seed, mode, monkeypatch):
    from pgw4era5_amd import settings
    var, src, trg = _interp_inputs(shape, seed, mode)
    assert var.dtype == np.float32 and src.dtype == trg.dtype == np.float64
    want = R.interp_logp_4d(var, src, trg, mode)
    c64 = O.interp_logp_4d(f64(var), src, trg, mode)
    assert not np.allclose(c64, want, rtol=1e-10, atol=1e-12, equal_nan=True)        # the input separates the two flows
    common64 = F.interp_logp_4d(f64(var), src, trg, mode)
    monkeypatch.setattr(settings, 'function_dtype_flow', 'reference')
    got = F.interp_logp_4d(var, src, trg, mode)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12, equal_nan=True)
    same(F.interp_logp_4d(f64(var), src, trg, mode), common64)                         # all float64: the bits of 'common'
    if mode != 'off':
        buf = np.zeros_like(want)
        F.interp_1d_for_timelatlon(var, np.log(src), np.log(trg), buf, var.shape[0], var.shape[2], var.shape[3], mode)
        want_l, _ = O.interp_columns_vectorised(np.log(src)[0].reshape(src.shape[1], -1), var[0].reshape(src.shape[1], -1),
                                                np.log(trg)[0].reshape(trg.shape[1], -1), mode)
        np.testing.assert_array_equal(buf[0].reshape(trg.shape[1], -1), want_l)      # arithmetic only: same bits
    with pytest.raises(NotImplementedError):
        F.interp_logp_4d(var, src.astype(f4), trg, mode)


@pytest.mark.parametrize('sfc', [True, False])
@pytest.mark.parametrize('shape,seed', DR.SHAPES)
def test_vert_interp_delta_float32_delta(F, shape, seed, sfc, monkeypatch):
    from pgw4era5_amd import settings
    c = DR.f32_case(shape, seed)
    era, plev = c['era'], np.asarray(c['plev'], dtype=np.float64)
    _, trg = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    delta = c['deltas']['ta'][3:4]
    if sfc:
        dsfc, psh = c['deltas']['tas'][3:4], c['deltas']['ps_hist'][3:4]
    else:
        dsfc = psh = None
        delta = (delta + np.random.default_rng(seed).normal(0, 1, delta.shape)).astype(f4)    # white noise with sign changes
    assert delta.dtype == np.float32
    want = R.vert_interp_delta(delta, plev, trg, dsfc, psh, True)
    c64 = R.vert_interp_delta(f64(delta), plev, trg, None if dsfc is None else f64(dsfc), None if psh is None else f64(psh), True)
    assert not np.allclose(c64, want, rtol=1e-10, atol=1e-12)                          # the input separates the two flows
    common64 = F.vert_interp_delta(f64(delta), trg, None if dsfc is None else f64(dsfc), None if psh is None else f64(psh), True, plev=plev)
    monkeypatch.setattr(settings, 'function_dtype_flow', 'reference')
    got = F.vert_interp_delta(delta, trg, dsfc, psh, True, plev=plev)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)
    same(F.vert_interp_delta(f64(delta), trg, None if dsfc is None else f64(dsfc), None if psh is None else f64(psh), True, plev=plev),
         common64)
    # era + delta in one call: float32 addend, float64 sum (step_03:170-173)
    got = F.vert_interp_delta(delta, trg, dsfc, psh, True, plev=plev, add_to=era['T'])
    np.testing.assert_allclose(got, era['T'] + want, rtol=1e-10, atol=1e-12)
    if sfc:        # every dtype of the two surface operands
        for a, b in ((f8, f4), (f4, f8), (f8, f8)):
            got = F.vert_interp_delta(delta, trg, dsfc.astype(a), psh.astype(b), True, plev=plev)
            np.testing.assert_allclose(got, R.vert_interp_delta(delta, plev, trg, dsfc.astype(a), psh.astype(b), True), rtol=1e-10, atol=1e-12)
        with pytest.raises(ValueError) as e:
            F.vert_interp_delta(delta, trg, dsfc, psh, False, plev=plev)
        assert 'ERA5 top pressure is lower than climate delta top pressure' in str(e.value)
    with pytest.raises(NotImplementedError):
        F.vert_interp_delta(delta, trg.astype(f4), dsfc, psh, True, plev=plev)


def test_time_lerp_integrate_tos_replace_delta_sfc_mixed(F, ref_flow, g32):
    rng = np.random.default_rng(11)
    vb, va = rng.normal(0, 3, (5, 7, 9)), rng.normal(0, 3, (5, 7, 9))
    x_hi = float(np.timedelta64(31, 'D').astype('timedelta64[ns]').astype(np.int64))
    x_new = float(np.timedelta64(10, 'D').astype('timedelta64[ns]').astype(np.int64))
    for a in (f4, f8):
        for b in (f4, f8):
            got = F.time_lerp(vb.astype(a), va.astype(b), x_hi, x_new)
            want = R.time_lerp(vb.astype(a), va.astype(b), '2006-01-01', '2006-02-01', '2006-01-11')
            same(got, want)                                                           # arithmetic only
    g = g32
    ops = (g['tos_tos'], g['tos_ts'], g['tos_land'], g['tos_ice'])
    for m in range(16):
        arrs = [x.astype(f4 if (m >> i) & 1 else f8) for i, x in enumerate(ops)]
        same(F.integrate_tos(*arrs), R.integrate_tos(*arrs))
    for d in (f4, f8):
        for s in (f4, f8):
            for h in (f4, f8):
                for i, ps in enumerate(g['rds_ps']):
                    P, D = F.replace_delta_sfc(g['rds_plev'], h(ps), g['rds_delta'].astype(d), s(9.25))
                    same(P, g['rds_out_P'][i])
                    same(D, g['rds_out_D'][i].astype(d))
    with pytest.raises(ValueError):
        F.replace_delta_sfc(g['rds_plev'], np.float32(50.0), g['rds_delta'], np.float32(9.25))      # ps_hist above the top level


def test_device_arrays_of_mixed_dtype(F, monkeypatch):
    from pgw4era5_amd import settings
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    era = DR.f32_case((7, 13, 21), 2)['era']
    _, pa = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    d_q, d_p, d_t = ctx.to_device(era['QV']), ctx.to_device(pa), ctx.to_device(era['T'])
    assert d_q.dtype == np.float32 and d_p.dtype == np.float64
    with pytest.raises(TypeError):
        F.specific_to_relative_humidity(d_q, d_p, d_t)
    monkeypatch.setattr(settings, 'function_dtype_flow', 'reference')
    got = F.specific_to_relative_humidity(d_q, d_p, d_t)
    assert got.dtype == np.float64 and got.shape == pa.shape
    same(got.numpy(), F.specific_to_relative_humidity(era['QV'], pa, era['T']))
    monkeypatch.setattr(settings, 'function_dtype_flow', 'neither')
    with pytest.raises(ValueError):
        F.specific_to_relative_humidity(d_q, d_p, d_t)


# ------------------------------------------------------------------ 6: import-swap rehearsal
def _rehearse(F, settings, monkeypatch, flow, c, inputs):
    monkeypatch.setattr(settings, 'function_dtype_flow', flow)
    return DR.rehearsal(F.relative_to_specific_humidity, lambda *a: F.integ_geopot(*a, full_column=False), c['era'], *inputs)


@pytest.mark.parametrize('shape,seed,ps_tol', [(s, k, 1.3e-7) for s, k in DR.SHAPES] + [((104, 1440, 137), 1, 6e-7)])
def test_import_swap_rehearsal(F, monkeypatch, shape, seed, ps_tol):
    """The reference's loop (step_03:182-319) with OUR relative_to_specific_humidity and integ_geopot on a float32 file."""
    from pgw4era5_amd import settings
    c = DR.f32_case(shape, seed)
    run, ta_pgw, hur_pgw, dzg = DR.oracle_file_run(c)
    got = _rehearse(F, settings, monkeypatch, 'reference', c, (ta_pgw, hur_pgw, dzg))
    ps_ref = f64(run['PS'])
    d_reference = np.max(np.abs(f64(got['PS']) - ps_ref) / ps_ref)
    print('   reference flow: n_iter %d (oracle %d), max |d max_err| %.3e, max rel dPS %.3e'
          % (got['n_iter'], run['n_iter'], np.max(np.abs(np.array(got['max_err'][:run['n_iter']]) - np.array(run['max_err'])[:got['n_iter']])),
             d_reference))
    assert got['n_iter'] == run['n_iter']
    if shape[0] == 104:
        assert run['n_iter'] == 7
    np.testing.assert_allclose(got['max_err'], run['max_err'], rtol=0, atol=2e-3)
    assert got['PS'].dtype == np.float32
    np.testing.assert_allclose(f64(got['PS']), ps_ref, rtol=ps_tol, atol=0)
    common = _rehearse(F, settings, monkeypatch, 'common', c, (ta_pgw, hur_pgw, dzg))
    d_common = np.max(np.abs(f64(common['PS']) - ps_ref) / ps_ref)
    print('   common flow:    n_iter %d, max rel dPS %.3e' % (common['n_iter'], d_common))
    assert d_reference <= d_common


# ------------------------------------------------------------------ 7: 'common' is untouched
def test_common_bits_survive_flipping_the_setting(F, monkeypatch):
    from pgw4era5_amd import settings
    c = DR.f32_case((7, 13, 21), 2)
    era = c['era']
    _, pa = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    pa_hl, _ = R.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    lvl = np.arange(1, 23)

    def run(dt):
        q, p, t, z, ph = era['QV'].astype(dt), pa.astype(dt), era['T'].astype(dt), era['FIS'].astype(dt), pa_hl.astype(dt)
        return [F.specific_to_relative_humidity(q, p, t), F.relative_to_specific_humidity(q * 1e4, p, t),
                F.integ_geopot(ph, z, t, q, lvl, 30000.0), F.interp_logp_4d(t, p, p * 1.003, 'constant'),
                F.time_lerp(t, t * 1.01, 3.0, 1.0), F.integrate_tos(z, z * 0.5, era['FR_LAND'].astype(dt), era['FR_SEA_ICE'].astype(dt)),
                F.specific_humidity_to_vapor_pressure(q, p), F.saturation_vapor_pressure_water_and_ice(p, t),
                F.vert_interp_delta(c['deltas']['ta'][:1].astype(dt), p, c['deltas']['tas'][:1].astype(dt),
                                    c['deltas']['ps_hist'][:1].astype(dt), True, plev=c['plev'])]
    assert settings.function_dtype_flow == 'common'
    before = [run(f4), run(f8)]
    monkeypatch.setattr(settings, 'function_dtype_flow', 'reference')
    mixed = F.specific_to_relative_humidity(era['QV'], pa, era['T'])
    assert mixed.dtype == np.float64
    monkeypatch.setattr(settings, 'function_dtype_flow', 'common')
    after = [run(f4), run(f8)]
    for bs, as_, dt in zip(before, after, (f4, f8)):
        for b, a in zip(bs, as_):
            assert b.dtype == dt
            same(a, b)
