"""GPU tests of the per-column reference level (settings.p_ref_inp = None, step_03:219-253) with the zg delta on a plev
axis of its own (pgw_file_args.nplev_zg / plev_zg): the CFday layout - ta / hur / ua / va on the reference's 99 levels, zg on
the 19 of Amon - against the oracles, and, on the cases of tests/local_pref_cases.py where the level moves and is held, bit
for bit against the same run with zg on the shared axis.  tests/test_wide_plev_host.py holds the CPU side of both."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_pref_cases as L                                                          # noqa: E402
import wide_plev_cases as W                                                           # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402

pytestmark = pytest.mark.gpu

# the default, one launch per pass (k_local_p_ref), and first launches of 1, 2, 3 passes (tests/test_local_pref_hip.py)
FORMS = (dict(), dict(multipass=0), dict(loop_guess=1), dict(loop_guess=2), dict(loop_guess=3))
REF_DTYPE = dict(f64=None, f32_fast=False, f32_reference=True)


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _scaled_qv_diff(a, b):
    scale = np.nanmax(np.abs(b), axis=(2, 3), keepdims=True)
    return np.nanmax(np.abs(a - b) / scale)


def _run(c, mode, opts=None, **kw):
    """pgw_for_era5_arrays(p_ref='local') with the case's own zg axis (c['plev_zg'], None: shared) under the context options
    `opts`, which are restored afterwards."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    old = {k: ctx.set_option(k, v) for k, v in (opts or {}).items()}
    try:
        return s3.pgw_for_era5_arrays(*L.args_of(c), p_ref='local', ref_dtype=REF_DTYPE[mode], plev_zg=c.get('plev_zg'), **kw)
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


# ================================================================== 1. 99 levels beside PLEV19, against the oracles
@pytest.mark.parametrize('mode', W.MODES)
@pytest.mark.parametrize('shape', W.SHAPES, ids=_id)
def test_zg_on_plev19_beside_99_levels_vs_oracle(shape, mode):
    """Tolerances: tests/test_local_pref_hip.py::test_moving_local_level_vs_oracle."""
    c = W.zg_case(shape, W.DTYPE[mode])
    want = W.zg_oracle(shape, mode)
    got = _run(c, mode)
    ps_w, qv_w = np.asarray(want['ps_pgw'], dtype=np.float64), want['hus_pgw']
    print('n_iter', got['n_iter'], want['n_iter'], 'max_err', got['max_err'], want['max_err'], 'levels', np.unique(want['p_ref']),
          'PS rel', np.max(np.abs(got['PS'].astype(np.float64) - ps_w) / ps_w), 'QV scaled', _scaled_qv_diff(got['QV'].astype(np.float64), qv_w))
    assert len(np.unique(want['p_ref'])) > 1
    assert got['n_iter'] == want['n_iter']
    if mode == 'f32_reference':
        np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=0, atol=2e-3)
        assert got['PS'].dtype == np.float32 and want['ps_pgw'].dtype == np.float32
        assert got['T'].dtype == np.float64 and got['QV'].dtype == np.float64
        np.testing.assert_allclose(got['PS'], want['ps_pgw'], rtol=1.3e-7, atol=0)
        np.testing.assert_allclose(got['T'], want['ta'], rtol=1e-9, atol=1e-9)
        assert _scaled_qv_diff(got['QV'], qv_w) < 6e-7
        return
    f64 = mode == 'f64'
    np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=1e-6 if f64 else 1e-5, atol=1e-7)
    np.testing.assert_allclose(got['PS'], want['ps_pgw'], rtol=1e-9 if f64 else 1e-6)
    np.testing.assert_allclose(got['QV'], want['hus_pgw'], rtol=1e-9 if f64 else 3e-6, atol=1e-18)


@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_loop_forms_are_bit_identical_on_the_cfday_layout(mode):
    """The multi-pass kernel with first launches of 1, 2 and 3 passes and the one-launch-per-pass form (k_local_p_ref): the
    same bits with the candidate table and the zg gather on zg's axis."""
    c = W.zg_case(W.SHAPES[0], W.DTYPE[mode])
    got = _run(c, mode)
    for opts in FORMS[1:]:
        alt = _run(c, mode, opts)
        assert alt['n_iter'] == got['n_iter'] and list(alt['max_err']) == list(got['max_err']), opts
        for k in ('PS', 'QV', 'T'):
            np.testing.assert_array_equal(alt[k], got[k], err_msg='%s %s' % (opts, k))


# ================================================================== 2. padding: an own axis that changes nothing
@pytest.mark.parametrize('dtype', L.DTYPES)
@pytest.mark.parametrize('shape', L.SHAPES, ids=_id)
def test_two_unreachable_levels_on_zg_axis_change_no_bit(shape, dtype):
    """ta-group and zg both on PLEV19, against the same run with 50 Pa and 20 Pa appended to zg's axis and records: the first
    match in file order never reaches them, so PS, QV, T, n_iter and max_err are the same bits - with nplev_zg != nplev, the
    gather's row count, continuation launches and the one-launch-per-pass form, where the level moves and is held."""
    c = L.build(shape, dtype)
    p = W.padded(c)
    for mode in (('f64',) if dtype == 'float64' else ('f32_fast', 'f32_reference')):
        for opts in FORMS:
            want = _run(c, mode, opts)
            got = _run(p, mode, opts)
            assert got['n_iter'] == want['n_iter'] and list(got['max_err']) == list(want['max_err']), (mode, opts)
            for k in ('PS', 'QV', 'T'):
                np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s %s' % (mode, opts, k))


@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_padded_zg_axis_under_i_reinterp(mode):
    c = L.build(L.SHAPES[0], W.DTYPE[mode])
    want = _run(c, mode, i_reinterp=True)
    got = _run(W.padded(c), mode, i_reinterp=True)
    assert got['n_iter'] == want['n_iter'] and list(got['max_err']) == list(want['max_err'])
    for k in ('PS', 'QV', 'T', 'U', 'V'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ================================================================== 3. the planned call
@pytest.mark.parametrize('layout', ['padded', 'cfday'])
def test_planned_call_takes_zg_axis(layout, monkeypatch):
    """process_file_device with reused `out` buffers goes through the file plan (pgw_step03_file_at), whose template carries
    nplev_zg / plev_zg: asserted taken, and the same bits as the host-built struct."""
    from pgw4era5_amd import _lib, step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    ctx._file_plans.clear()
    c = W.padded(L.build(L.SHAPES[1], 'float64')) if layout == 'padded' else W.zg_case(W.SHAPES[1], 'float64')
    dtype = np.dtype('float64')
    ds = s3.DeltaSet(ctx, c['deltas'], c['delta_times'], c['plev'], dtype)
    ds.plev_zg = np.ascontiguousarray(c['plev_zg'])
    calls = {'pgw_step03_file': 0, 'pgw_step03_file_at': 0}

    def counted(name, real):
        def call(*a):
            calls[name] += 1
            return real(*a)
        return call
    for name in calls:
        monkeypatch.setattr(ctx.lib, name, counted(name, getattr(ctx.lib, name)))
    try:
        era = s3._upload_era(ctx, c['era'], dtype)
        coeffs = dict(ak=c['era']['ak'], bk=c['era']['bk'], soil1=c['era']['soil1'])
        res = {}
        for plan in ('1', '0', '1'):
            monkeypatch.setenv('PGW_FILE_PLAN', plan)
            out = res.setdefault(plan, {})
            before = dict(calls)
            o, info = s3.process_file_device(ctx, era, coeffs, ds, c['target_dt'], True, p_ref='local', out=out)
            used = [k for k in calls if calls[k] != before[k]]
            assert used == ['pgw_step03_file_at' if plan == '1' else 'pgw_step03_file'], (plan, used)
            a = _lib.FileArgs.from_buffer_copy(ctx._last_file_args)
            assert a.local_p_ref == 1 and a.nplev_zg == len(c['plev_zg']) and a.nplev == len(c['plev'])
            table = C.cast(a.plev_zg, C.POINTER(C.c_double))
            assert [table[i] for i in range(a.nplev_zg)] == list(c['plev_zg'])
            res[plan + 'info'] = info
            res[plan + 'host'] = {k: o[k].numpy() for k in ('PS', 'T', 'QV', 'U', 'V')}
        assert res['1info']['n_iter'] == res['0info']['n_iter'] and res['1info']['max_err'] == res['0info']['max_err']
        for k in ('PS', 'T', 'QV', 'U', 'V'):
            np.testing.assert_array_equal(res['1host'][k], res['0host'][k], err_msg=k)
    finally:
        ds.free()
        ctx._file_plans.clear()


# ================================================================== 4. errors
@pytest.mark.parametrize('opts', FORMS, ids=lambda o: '-'.join('%s%d' % kv for kv in o.items()) or 'default')
def test_no_level_found_on_a_cut_zg_axis(opts):
    """local_pref_cases.error_case() with ta / hur / ua / va back on the full PLEV19 and only zg on the cut axis
    (plev >= 85000 Pa): pass 1 finds a level for every column, a later pass none for one - `No reference pressure level`
    (status 19), decided on zg's axis."""
    from pgw4era5_amd import synthetic
    e = L.error_case()
    full = synthetic.make_case(4, 5, 12, seed=22)
    d = dict(e['deltas'])
    for k in ('ta', 'hur', 'ua', 'va'):
        d[k] = full['deltas'][k]
    c = dict(e, deltas=d, plev=full['plev'], plev_zg=np.asarray(e['plev'], dtype=np.float64))
    assert len(c['plev_zg']) == 3 and d['zg'].shape[1] == 3 and d['ta'].shape[1] == 19
    with pytest.raises(ValueError, match='No reference pressure level') as ei:
        _run(c, 'f64', opts)
    assert 'lies below the surface' not in str(ei.value)
    assert ei.value.status == 19


def test_limits_of_zg_axis():
    """More than 64 levels on zg's axis under p_ref = None: ValueError before any launch; a fixed p_ref that is no level of
    zg's axis: KeyError, as before."""
    c = W.zg_case(W.SHAPES[0], 'float64')
    wide = dict(c, deltas=dict(c['deltas'], zg=np.zeros((12, 65) + c['deltas']['zg'].shape[2:])), plev_zg=np.geomspace(100000.0, 100.0, 65))
    with pytest.raises(ValueError, match='1 to 64 levels'):
        _run(wide, 'f64')
    from pgw4era5_amd import step_03_apply_to_era as s3
    with pytest.raises(KeyError):
        s3.pgw_for_era5_arrays(*L.args_of(c), p_ref=32500.0, plev_zg=c['plev_zg'])      # a level of the 99-level axis only
    ok = s3.pgw_for_era5_arrays(*L.args_of(c), p_ref=30000.0, plev_zg=c['plev_zg'])      # on both axes: selected on zg's
    assert ok['n_iter'] >= 1 and np.isfinite(ok['PS']).all()
