"""GPU tests of the per-column reference level (settings.p_ref_inp = None, step_03:219-253, functions.py:583-598) on the
cases of tests/local_pref_cases.py, where the level moves and is held back after the first pass (test_local_pref_host.py
proves that on the CPU): k_local_p_ref in the one-launch-per-pass form and under i_reinterp, the LOCAL branch of
k_ps_loop_multi and its continuation launches - against the oracles, and the loop forms against each other bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_pref_cases as L                                                          # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ('f64', 'f32_fast', 'f32_reference')
DTYPE = dict(f64='float64', f32_fast='float32', f32_reference='float32')
# the default, one launch per pass (k_local_p_ref), and first launches of 1, 2, 3 passes: a level change or a held column
# then falls on the first pass of a continuation launch or in the middle of a launch; continuation launches take 2 passes
FORMS = (dict(), dict(multipass=0), dict(loop_guess=1), dict(loop_guess=2), dict(loop_guess=3))
_cache = {}


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _scaled_qv_diff(a, b):
    """max |a - b| relative to each level's largest value (tests/test_hip_parity.py)."""
    scale = np.nanmax(np.abs(b), axis=(2, 3), keepdims=True)
    return np.nanmax(np.abs(a - b) / scale)


def _run(c, mode, opts=None, **kw):
    """pgw_for_era5_arrays(p_ref='local') under the context options `opts`, which are restored afterwards."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    old = {k: ctx.set_option(k, v) for k, v in (opts or {}).items()}
    try:
        return s3.pgw_for_era5_arrays(*L.args_of(c), p_ref='local', ref_dtype=None if mode == 'f64' else mode == 'f32_reference',
                                      **kw)
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def _default_run(shape, mode, adj_factor):
    """The default form's result, computed once per case (call with settings.adj_factor already set)."""
    key = (shape, mode, adj_factor)
    if key not in _cache:
        _cache[key] = _run(L.build(shape, DTYPE[mode]), mode)
    return _cache[key]


@pytest.mark.parametrize('adj_factor', L.ADJ_FACTORS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', L.SHAPES, ids=_id)
def test_moving_local_level_vs_oracle(shape, mode, adj_factor, monkeypatch):
    """float64 file and float32 file in fast mode against O.adjust_ps_loop_local_pref on the composition
    test_local_p_ref_mode_vs_oracle uses; float32 file in reference-dtype mode against R.pgw_for_era5_arrays(p_ref=None).
    Tolerances: those of test_local_p_ref_mode_vs_oracle and test_reference_dtype_mode_vs_refdtype_oracle."""
    import pgw4era5_amd.settings as S
    monkeypatch.setattr(S, 'adj_factor', adj_factor)
    c = L.build(shape, DTYPE[mode])
    got = _default_run(shape, mode, adj_factor)
    if mode == 'f32_reference':
        want = R.pgw_for_era5_arrays(*L.args_of(c), p_ref=None, adj_factor=adj_factor)
        print('n_iter', got['n_iter'], want['n_iter'], 'max_err', got['max_err'], want['max_err'],
              'PS rel', np.max(np.abs(got['PS'].astype(np.float64) - want['PS']) / want['PS']),
              'QV scaled', _scaled_qv_diff(got['QV'], want['QV']))
        assert got['n_iter'] == want['n_iter']
        np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=0, atol=2e-3)
        assert got['PS'].dtype == np.float32 and want['PS'].dtype == np.float32
        assert got['T'].dtype == np.float64 and got['QV'].dtype == np.float64
        np.testing.assert_allclose(got['PS'], want['PS'], rtol=1.3e-7, atol=0)
        np.testing.assert_allclose(got['T'], want['T'], rtol=1e-9, atol=1e-9)
        assert _scaled_qv_diff(got['QV'], want['QV']) < 6e-7
        return
    want, _ = L.oracle_run(shape, DTYPE[mode], adj_factor)
    print('n_iter', got['n_iter'], want['n_iter'], 'max_err', got['max_err'], want['max_err'],
          'PS rel', np.max(np.abs(got['PS'].astype(np.float64) - want['ps_pgw']) / want['ps_pgw']),
          'QV rel', np.nanmax(np.abs(got['QV'].astype(np.float64) - want['hus_pgw']) / np.abs(want['hus_pgw'])))
    assert got['n_iter'] == want['n_iter']
    f64 = mode == 'f64'
    np.testing.assert_allclose(got['max_err'], want['max_err'], rtol=1e-6 if f64 else 1e-5, atol=1e-7)
    np.testing.assert_allclose(got['PS'], want['ps_pgw'], rtol=1e-9 if f64 else 1e-6)
    np.testing.assert_allclose(got['QV'], want['hus_pgw'], rtol=1e-9 if f64 else 3e-6, atol=1e-18)


@pytest.mark.parametrize('adj_factor', L.ADJ_FACTORS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', L.SHAPES, ids=_id)
def test_loop_forms_are_bit_identical_on_a_moving_level(shape, mode, adj_factor, monkeypatch):
    import pgw4era5_amd.settings as S
    monkeypatch.setattr(S, 'adj_factor', adj_factor)
    c = L.build(shape, DTYPE[mode])
    got = _default_run(shape, mode, adj_factor)
    for opts in FORMS[1:]:
        alt = _run(c, mode, opts)
        assert alt['n_iter'] == got['n_iter'], opts
        assert alt['max_err'] == got['max_err'], opts
        for k in ('PS', 'QV', 'T'):
            np.testing.assert_array_equal(alt[k], got[k], err_msg='%s %s' % (opts, k))


@pytest.mark.parametrize('adj_factor', L.ADJ_FACTORS)
@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_reinterp_with_a_moving_local_level_vs_oracle(mode, adj_factor, monkeypatch):
    """settings.i_reinterp = 1 calls k_local_p_ref in every pass.  Tolerances: test_reinterp_mode_vs_oracle's."""
    import pgw4era5_amd.settings as S
    monkeypatch.setattr(S, 'adj_factor', adj_factor)
    c = L.build(L.SHAPES[0], DTYPE[mode])
    got = _run(c, mode, i_reinterp=True)
    if mode == 'f32_reference':
        want = R.pgw_for_era5_arrays_reinterp(*L.args_of(c), p_ref=None, adj_factor=adj_factor)
        tol = dict(PS=2.5e-7, QV=6e-7)
    else:
        want = O.pgw_for_era5_arrays_reinterp(*L.args_of(c), p_ref=None, adj_factor=adj_factor)
        tol = dict(PS=1e-9, QV=1e-9)
    scale = np.nanmax(np.abs(want['QV']), axis=(2, 3), keepdims=True)
    qv = np.nanmax(np.abs(got['QV'] - want['QV']) / scale)
    print('n_iter', got['n_iter'], want['n_iter'], 'max_err', got['max_err'], want['max_err'],
          'PS rel', np.max(np.abs(got['PS'].astype(np.float64) - want['PS']) / want['PS']), 'QV scaled', qv)
    assert len(np.unique(want['p_ref'])) > 1
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


@pytest.mark.parametrize('opts', FORMS, ids=lambda o: '-'.join('%s%d' % kv for kv in o.items()) or 'default')
def test_a_level_lost_in_a_later_pass_raises_the_reference_error(opts):
    """Pass 1 finds a level for every column, pass 2 none for one: `No reference pressure level` and nothing else - the
    column's NaN level, with which the same pass also integrates, must not surface as `p_ref locally lies below the
    surface`."""
    c, i = L.error_case(), L.loop_inputs()
    with pytest.raises(ValueError, match='No reference pressure level'):
        O.adjust_ps_loop_local_pref(i['ak'], i['bk'], i['akm'], i['bkm'], i['PS'], i['FIS'], i['T'], i['QV'], i['ta'], i['hur'],
                                    i['zg'], i['plev'])
    with pytest.raises(ValueError, match='No reference pressure level') as e:
        _run(c, 'f64', opts)
    assert 'lies below the surface' not in str(e.value)
