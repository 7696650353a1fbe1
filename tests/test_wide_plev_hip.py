"""GPU tests of delta pressure axes of more than 64 levels (the 128-entry plev table of the delta kernels) on the cases of
tests/wide_plev_cases.py; test_wide_plev_host.py proves on the CPU that their targets fall on both sides of source index
64, that every column of the 99-level case inserts the surface beyond it and that some ps_hist lie above all levels.
S = 64 is the last axis of the 64-entry table, S = 65 the first of the wide one: both are held to the function-level
entries bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_plev_cases as W                                                           # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = W.SHAPES[0]
TOP_MSG = 'ERA5 top pressure is lower than climate delta top pressure'


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _scaled_diff(a, b):
    """max |a - b| relative to each level's largest value (tests/test_hip_parity.py)."""
    scale = np.nanmax(np.abs(b), axis=(2, 3), keepdims=True)
    return np.nanmax(np.abs(a - b) / scale)


def _file(c, mode, ignore_top=True, opts=None, deltas=None, **kw):
    """pgw_for_era5_arrays with the fixed reference level under the context options `opts`, which are restored afterwards."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    old = {k: ctx.set_option(k, v) for k, v in (opts or {}).items()}
    try:
        return s3.pgw_for_era5_arrays(c['era'], c['deltas'] if deltas is None else deltas, c['delta_times'], c['plev'], c['target_dt'],
                                      ignore_top, p_ref=W.P_REF, ref_dtype=dict(f64=None, f32_fast=False, f32_reference=True)[mode], **kw)
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


# ================================================================== 1. the file path against the oracles
@pytest.mark.parametrize('shape', W.SHAPES, ids=_id)
@pytest.mark.parametrize('mode', W.MODES)
@pytest.mark.parametrize('S', W.WIDE)
def test_file_path_vs_oracle(S, mode, shape):
    """Tolerances: tests/test_hip_parity.py::test_whole_file_vs_oracle (float64 file; float32 file in fast mode) and
    ::test_reference_dtype_mode_vs_refdtype_oracle (float32 file, reference-dtype mode), max_err as in
    tests/test_local_pref_hip.py::test_moving_local_level_vs_oracle.  RELHUM_pgw in reference-dtype mode carries the
    float32 e_sat chain of the ERA state (device expf against numpy's) like QV does, and takes QV's bound."""
    c = W.build(shape, S, W.DTYPE[mode])
    want = W.oracle_file(shape, S, mode)
    got = _file(c, mode)
    print('n_iter', got['n_iter'], want['n_iter'], 'max_err', got['max_err'], want['max_err'],
          'PS rel', np.max(np.abs(got['PS'].astype(np.float64) - want['PS']) / want['PS']),
          'T abs', np.max(np.abs(got['T'] - want['T'])), 'QV scaled', _scaled_diff(got['QV'].astype(np.float64), want['QV']),
          'hur scaled', _scaled_diff(got['RELHUM_pgw'].astype(np.float64), want['RELHUM_pgw']))
    assert got['n_iter'] == want['n_iter'] == 6
    if mode == 'f32_reference':
        np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=0, atol=2e-3)
        for k in ('T', 'QV', 'U', 'V', 'RELHUM_pgw'):
            assert got[k].dtype == np.float64 and want[k].dtype == np.float64, k
        assert got['PS'].dtype == np.float32 and want['PS'].dtype == np.float32
        np.testing.assert_allclose(got['PS'], want['PS'], rtol=1.3e-7, atol=0, err_msg='PS')
        for k in ('T', 'U', 'V'):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-9, err_msg=k)
        assert _scaled_diff(got['QV'], want['QV']) < 6e-7
        assert _scaled_diff(got['RELHUM_pgw'], want['RELHUM_pgw']) < 6e-7
        return
    f64 = mode == 'f64'
    np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=1e-6 if f64 else 1e-5, atol=1e-7)
    tol = 1e-9 if f64 else 1e-6
    for k in ('PS', 'T', 'U', 'V', 'RELHUM_pgw'):
        np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=1e-5 if (not f64 and k in ('U', 'V', 'RELHUM_pgw')) else 1e-12,
                                   err_msg=k)
    np.testing.assert_allclose(got['QV'], want['QV'], rtol=tol if f64 else 3e-6, atol=1e-12)


# ================================================================== 2. the same bits as the function-level entries
@pytest.mark.parametrize('shape', W.SHAPES, ids=_id)
@pytest.mark.parametrize('S', [64, 65])
def test_file_path_is_the_function_level_composition_bit_for_bit(S, shape):
    """include/pgw_hip.h: "Results are identical to calling the function-level entry points in the reference's order" - on
    the last axis of the narrow table and the first of the wide one: time_lerp, vert_interp_delta (+ add_to),
    specific_to_relative_humidity and adjust_ps_loop of pgw4era5_amd.functions against one pgw_step03_file."""
    from pgw4era5_amd import functions as F
    c = W.build(shape, S, 'float64')
    era, d, plev = c['era'], c['deltas'], c['plev']
    got = _file(c, 'f64')
    from pgw4era5_amd import step_03_apply_to_era as s3
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(c['delta_times'], c['target_dt'])
    assert x_hi != 0.0
    ld = lambda k: F.time_lerp(d[k][keep[ib]][None], d[k][keep[ia]][None], x_hi, x_new)
    from pgw4era5_amd import _lib
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    N = era['T'].shape[1]
    akm, bkm = np.empty(N), np.empty(N)                    # the full-level coefficients the kernels use
    ctx._check(ctx.lib.pgw_get_full_level_coeffs(ctx.handle, akm.ctypes.data_as(_lib._dp), bkm.ctypes.data_as(_lib._dp)))
    pa = akm[None, :, None, None] + era['PS'][:, None] * bkm[None, :, None, None]
    relhum = F.specific_to_relative_humidity(era['QV'], pa, era['T'])
    psh = ld('ps_hist')
    ta = F.vert_interp_delta(ld('ta'), pa, ld('tas'), psh, True, plev=plev, add_to=era['T'])
    hur = F.vert_interp_delta(ld('hur'), pa, ld('hurs'), psh, True, plev=plev, add_to=relhum)
    ua = F.vert_interp_delta(ld('ua'), pa, None, None, True, plev=plev, add_to=era['U'])
    va = F.vert_interp_delta(ld('va'), pa, None, None, True, plev=plev, add_to=era['V'])
    kref = int(np.nonzero(plev == W.P_REF)[0][0])
    loop = F.adjust_ps_loop(era['ak'], era['bk'], era['PS'], era['FIS'], era['T'], era['QV'], ta, hur, ld('zg')[:, kref], p_ref=W.P_REF)
    for name, want in (('T', ta), ('RELHUM_pgw', hur), ('U', ua), ('V', va), ('PS', loop['ps_pgw']), ('QV', loop['hus_pgw'])):
        np.testing.assert_array_equal(got[name], want, err_msg=name)
    assert got['n_iter'] == loop['n_iter'] and list(got['max_err']) == list(loop['max_err'])


def test_kernel_variants_agree_on_the_wide_table():
    """PGW_OPT_QUAD = 0 (the pair kernels), 64-bit offsets, no fused first pass and the loop forms of
    tests/test_local_pref_hip.py: the same bits as the default on the 99-level axis, for every storage mode."""
    import test_local_pref_hip as TL
    for mode in W.MODES:
        c = W.build(SMALL, 99, W.DTYPE[mode])
        got = _file(c, mode)
        variants = list(TL.FORMS[1:]) + [dict(force_off64=1)] + ([dict(fused_first=0)] if mode == 'f64' else [])
        for opts in variants:
            alt = _file(c, mode, opts=opts)
            assert alt['n_iter'] == got['n_iter'] and list(alt['max_err']) == list(got['max_err']), (mode, opts)
            for k in ('PS', 'QV', 'T', 'U', 'V'):
                np.testing.assert_array_equal(alt[k], got[k], err_msg='%s %s %s' % (mode, opts, k))
        if mode != 'f32_reference':                      # the pair kernels have no reference-dtype form
            alt = _file(c, mode, opts=dict(quad=0))
            assert alt['n_iter'] == got['n_iter']
            for k in ('T', 'U', 'V', 'PS'):
                np.testing.assert_array_equal(alt[k], got[k], err_msg='%s quad=0 %s' % (mode, k))


# ================================================================== 3. i_reinterp, the deltas themselves, function level
@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_reinterp_on_99_levels_vs_oracle(mode):
    """settings.i_reinterp = 1 (k_reinterp_pair on the wide table) against the oracles' _reinterp forms.  Tolerances: those of
    tests/test_local_pref_hip.py::test_reinterp_with_a_moving_local_level_vs_oracle."""
    c = W.build(SMALL, 99, W.DTYPE[mode])
    want = W.oracle_file(SMALL, 99, mode, reinterp=True)
    got = _file(c, mode, i_reinterp=True)
    tol = dict(PS=2.5e-7, QV=6e-7) if mode == 'f32_reference' else dict(PS=1e-9, QV=1e-9)
    qv = _scaled_diff(got['QV'], want['QV'])
    print('n_iter', got['n_iter'], want['n_iter'], 'max_err', got['max_err'], want['max_err'],
          'PS rel', np.max(np.abs(got['PS'].astype(np.float64) - want['PS']) / want['PS']), 'QV scaled', qv)
    assert got['n_iter'] == want['n_iter']
    np.testing.assert_allclose(np.asarray(got['max_err']), np.asarray(want['max_err']), rtol=1e-6 if mode == 'f64' else 0.2, atol=1e-7)
    np.testing.assert_allclose(got['PS'], want['PS'], rtol=tol['PS'], err_msg='PS')
    if mode == 'f32_reference':
        assert got['T'].dtype == np.float64 and got['QV'].dtype == np.float64 and got['PS'].dtype == np.float32
        np.testing.assert_allclose(got['T'], want['T'], rtol=6e-8, err_msg='T')
        for k in ('U', 'V'):
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=2e-5, err_msg=k)
    else:
        for k in ('T', 'U', 'V'):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-9, err_msg=k)
    assert qv < tol['QV']


@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_delta_fields_on_99_levels_vs_oracle(mode):
    """`-D interpolate_full`: pgw_delta_fields against the oracle's vert_interp_delta of the four variables; rtol = atol = 1e-9
    as in tests/test_step03_debug_hip.py::test_delta_fields_vs_oracle."""
    from pgw4era5_amd import step_03_apply_to_era as s3, step_03_debug as dbg
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    dtype = np.dtype(W.DTYPE[mode])
    c = W.build(SMALL, 99, W.DTYPE[mode])
    era, d = c['era'], c['deltas']
    M = R if mode == 'f32_reference' else O
    _, pa = M.hybrid_pressure(era['ak'], era['bk'], era['PS'] if M is R else np.asarray(era['PS'], dtype=np.float64))
    ld = lambda k: M.load_delta_values(d[k], c['delta_times'], c['target_dt'])
    ctx.set_levels(era['ak'], era['bk'], era.get('akm'), era.get('bkm'))
    ds = s3.DeltaSet(ctx, d, c['delta_times'], c['plev'], dtype)
    try:
        ps = ctx.to_device(np.ascontiguousarray(era['PS'], dtype=dtype), dtype)
        out = dbg.delta_fields_device(ctx, ps, ds, c['target_dt'], era['T'].shape[1], mode == 'f32_reference', True)
        got = {k: v.numpy() for k, v in out.items()}
    finally:
        ds.free()
    for var in ('ta', 'hur', 'ua', 'va'):
        sfc, psh = (ld(var + 's'), ld('ps_hist')) if var in ('ta', 'hur') else (None, None)
        want = M.vert_interp_delta(ld(var), c['plev'], pa, sfc, psh, True)
        assert got[var].dtype == np.float64
        np.testing.assert_allclose(got[var], want, rtol=1e-9, atol=1e-9, err_msg=var)


def test_function_level_entries_on_99_levels_vs_oracle():
    """functions.vert_interp_delta (pgw_vert_interp_delta) and functions.replace_delta_sfc on the 99-level axis; tolerances
    of tests/test_hip_parity.py::test_vert_interp_delta_vs_oracle."""
    from pgw4era5_amd import functions as F
    c = W.build(SMALL, 99, 'float64')
    era, d, plev = c['era'], c['deltas'], c['plev']
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    for sfc, psh in ((d['tas'][3:4], d['ps_hist'][3:4]), (None, None)):
        want = O.vert_interp_delta(d['ta'][3:4], plev, pa, sfc, psh, ignore_top_pressure_error=True)
        got = F.vert_interp_delta(d['ta'][3:4], pa, sfc, psh, ignore_top_pressure_error=True, plev=plev)
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-13)
    asc = plev[::-1]
    col = d['ta'][3, ::-1, 1, 2]
    for ps_hist in (float(d['ps_hist'][3, 1, 2]), 101000.5, float(asc[70]), float(asc[64]), float(asc[1])):
        wp, wd = O.replace_delta_sfc(asc, ps_hist, col, 1.25)
        gp, gd = F.replace_delta_sfc(asc, ps_hist, col, 1.25)
        np.testing.assert_array_equal(gp, wp)
        np.testing.assert_array_equal(gd, wd)
    for f in (O.replace_delta_sfc, F.replace_delta_sfc):      # ps_hist on min(plev): np.max of an empty argwhere (:362-365)
        with pytest.raises(ValueError):
            f(asc, float(asc[0]), col, 1.25)


# ================================================================== 4. checks and errors on the wide table
def test_model_top_check_on_the_wide_table():
    """The 99-level axes that end at about 115 Pa lie below the synthetic model top (0.5 Pa): without
    --ignore_top_pressure_error the reference's ValueError; the axis that reaches 0.4 Pa passes, with the same result as with
    the check off."""
    c = W.build(SMALL, 99, 'float64')
    with pytest.raises(ValueError, match=TOP_MSG):
        O.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], False, p_ref=W.P_REF)
    for kw in (dict(), dict(i_reinterp=True)):
        with pytest.raises(ValueError, match=TOP_MSG):
            _file(c, 'f64', ignore_top=False, **kw)
    hi = W.build(SMALL, 99, 'float64', top=0.4)
    checked = _file(hi, 'f64', ignore_top=False)
    free = _file(hi, 'f64', ignore_top=True)
    assert checked['n_iter'] == free['n_iter']
    for k in ('PS', 'T', 'QV', 'U', 'V'):
        np.testing.assert_array_equal(checked[k], free[k], err_msg=k)


def test_ps_hist_above_the_top_delta_level_is_status_15():
    """ps_hist below min(plev) in one column: the bare ValueError of replace_delta_sfc (functions.py:360-361) for that column -
    sfc_level and the tuned kernels' own text of the rule on the wide table."""
    c = W.build(SMALL, 99, 'float64')
    nlat, nlon, _ = SMALL
    col = 2 * nlon + 4
    d = dict(c['deltas'], ps_hist=c['deltas']['ps_hist'].copy())
    d['ps_hist'].reshape(12, -1)[:, col] = 0.5 * c['plev'].min()
    for opts, kw in ((None, {}), (dict(quad=0), {}), (None, dict(i_reinterp=True))):
        with pytest.raises(ValueError) as e:
            _file(c, 'f64', deltas=d, opts=opts, **kw)
        assert str(e.value) == '' and e.value.column == col, (opts, kw)


def test_more_than_128_levels_is_a_value_error():
    from pgw4era5_amd import _lib, functions as F, step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    nlat, nlon, nlev = SMALL
    from pgw4era5_amd import synthetic
    c = synthetic.make_case(nlat, nlon, nlev, seed=1, plev=np.geomspace(101000.0, 120.0, 129))
    with pytest.raises(ValueError, match=r'\[2, 128\]'):
        s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True, p_ref=c['plev'][40])
    _, pa = O.hybrid_pressure(c['era']['ak'], c['era']['bk'], c['era']['PS'])
    with pytest.raises(ValueError, match=r'\[2, 128\]'):
        F.vert_interp_delta(c['deltas']['ta'][:1], pa, plev=c['plev'], ignore_top_pressure_error=True)
    # the library's own check, for a caller of the C-ABI
    plev = np.ascontiguousarray(c['plev'][::-1])
    a = ctx.to_device(np.zeros((1, 129, 1)), np.dtype('float64'))
    s = ctx.to_device(np.zeros((1, 1)), np.dtype('float64'))
    rc = ctx.lib.pgw_replace_delta_sfc(ctx.handle, _lib.PGW_F64, 1, 129, 1, plev.ctypes.data_as(_lib._dp), a.ptr, s.ptr, s.ptr, a.ptr, a.ptr)
    assert rc == _lib.PGW_ERR_ARG
    with pytest.raises(ValueError, match=r'nplev must be in \[1, 128\]'):
        ctx._check(rc)
