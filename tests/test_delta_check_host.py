"""CPU tests of the delta check (pgw4era5_amd/check_deltas.py): the conditions of the cases (tests/delta_check_cases.py), the
numpy statement by hand, the table and its formatting, the command line and file-name rule, the errors raised before any
`pgw_*` call, and the C entry's declaration and binding."""
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_check_cases as K                                                        # noqa: E402
from function_recorder import RecordingContext                                       # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conditions_of_the_cases():
    shares = K.conditions()
    assert shares[((7, 9), 12, 'state')] > 0.19                  # 100000 Pa of PLEV5 is NaN in every column: a fifth at least


# ---- the statement ------------------------------------------------------------------------------------------------------
def test_statement_by_hand_on_a_two_level_column():
    ak, bk = np.array([0.0, 20000.0, 0.0]), np.array([0.0, 0.0, 1.0])          # akm = 10000, 10000; bkm = 0, 0.5
    ps = np.array([[[100000.0]]])
    akm, bkm = O.full_level_coeffs(ak, bk)
    assert akm.tolist() == [10000.0, 10000.0] and bkm.tolist() == [0.0, 0.5]
    pa = np.array([10000.0, 60000.0])
    T, q, u, v = (np.array(x).reshape(1, 2, 1, 1) for x in ([220.0, 270.0], [1e-5, 4e-3], [30.0, -6.0], [-2.0, 5.0]))
    plev = np.array([60000.0, 30000.0, 10000.0, 5000.0, 70000.0])
    got = K.state_on_plev(ps, T, q, u, v, ak, bk, plev)[:, 0, :, 0, 0]
    rh = O.specific_to_relative_humidity(q[0, :, 0, 0], pa, T[0, :, 0, 0])
    w = (np.log(30000.0) - np.log(10000.0)) / (np.log(60000.0) - np.log(10000.0))
    for i, x in enumerate(([220.0, 270.0], rh, [30.0, -6.0], [-2.0, 5.0])):
        assert got[i, 0] == x[1] and got[i, 2] == x[0]                         # exact hits: the level's value itself
        assert np.isnan(got[i, 3]) and np.isnan(got[i, 4])                     # above the top, below the lowest full level
        np.testing.assert_allclose(got[i, 1], x[0] + w * (x[1] - x[0]), rtol=1e-14)
    assert got[2, 1] * 30.0 > -180.0 and -6.0 < got[2, 1] < 30.0               # the wind crosses zero inside the bracket
    # two states and the mask: error = change - delta strictly above ps_hist, NaN at and below
    b = (ps + 100.0, T + 1.0, q, u + 2.0, v)
    rec = {n: np.full((1, 5, 1, 1), 0.5) for n in K.VARS}
    rec['ps_hist'] = np.full((1, 1, 1), 30000.0)
    times = {n: np.array(['1995-08-02T03:00:00'], dtype='datetime64[s]') for n in rec}
    change = K.state_change((ps, T, q, u, v), b, ak, bk, plev)
    err = K.state_error((ps, T, q, u, v), b, ak, bk, plev, rec, times, np.datetime64('2006-08-02T03:00:00'))
    assert change[0, 0, 2, 0, 0] == 1.0 and change[2, 0, 2, 0, 0] == 2.0       # the pure-pressure level does not move
    assert err[0, 0, 2, 0, 0] == 0.5 and err[2, 0, 2, 0, 0] == 1.5
    assert np.isnan(err[:, 0, 1]).all() and np.isnan(err[:, 0, 0]).all()       # p == ps_hist and below it: masked


def test_edge_columns_of_the_statement():
    e = K.edge_case()
    col = {n: i for i, n in enumerate(e['names'])}
    lev = {p: i for i, p in enumerate(e['plev'])}
    a, b = K.fields(e['a']), K.fields(e['b'])
    xa = K.state_on_plev(*a, e['ak'], e['bk'], e['plev'])[:, 0, :, 0, :]
    change = K.state_change(a, b, e['ak'], e['bk'], e['plev'])[:, 0, :, 0, :]
    times = {n: e['times'] for n in e['deltas']}
    err = K.state_error(a, b, e['ak'], e['bk'], e['plev'], e['deltas'], times, e['target'])[:, 0, :, 0, :]
    assert xa[0, lev[10000.0], col['plain']] == e['a']['T'][0, 2, 0, col['plain']]              # X[k] itself
    assert xa[2, lev[1000.0], col['plain']] == e['a']['U'][0, 0, 0, col['plain']]               # ... at k = 0 too
    assert np.isnan(xa[:, lev[500.0]]).all() and np.isnan(xa[:, lev[100000.0]]).all()
    assert np.isnan(change[:, lev[85000.0], col['low_in_a']]).all() and np.isfinite(change[:, lev[85000.0], col['plain']]).all()
    assert np.isnan(err[:, lev[50000.0], col['psh_on_level']]).all() and np.isfinite(err[:, lev[40000.0], col['psh_on_level']]).all()
    assert np.isfinite(err[:, lev[50000.0], col['psh_ulp_above']]).all() and np.isnan(err[:, lev[50000.0], col['psh_ulp_below']]).all()
    assert np.isnan(err[:, :, col['psh_nan']]).all() and np.isfinite(change[:, lev[50000.0], col['psh_nan']]).all()
    assert np.isnan(xa[:, :, col['ps_nan']]).all() and np.isnan(change[:, :, col['descending']]).all()
    nan_t = np.isnan(xa[0, :, col['t_nan']]) & ~np.isnan(xa[0, :, col['plain']])
    assert nan_t.sum() >= 2 and np.array_equal(np.isnan(xa[1, :, col['t_nan']]), np.isnan(xa[0, :, col['t_nan']]))
    assert np.array_equal(np.isnan(xa[2, :, col['t_nan']]), np.isnan(xa[2, :, col['plain']]))   # the winds do not see T
    u = xa[2, :, col['wind_sign']]
    assert (u[np.isfinite(u)] > 0).any() and (u[np.isfinite(u)] < 0).any()
    top = K.edge_case(hybrid_top=True)
    ct = K.state_change(K.fields(top['a']), K.fields(top['b']), top['ak'], top['bk'], top['plev'])[:, 0, :, 0, :]
    xt = K.state_on_plev(*K.fields(top['a']), top['ak'], top['bk'], top['plev'])[:, 0, :, 0, :]
    assert np.isfinite(xt[:, lev[500.0], col['low_in_a']]).all() and np.isnan(ct[:, lev[500.0], col['low_in_a']]).all()


# ---- tables and formatting -----------------------------------------------------------------------------------------------
def test_table_and_formatting():
    from pgw4era5_amd import check_deltas as C, check_geopot as G
    t = G.table_from_partials([100000.0, 30000.0], [0, 4], [0.0, 2.0], [0.0, 3.0], [0.0, 1.25])
    for var in C.VARS:
        text = C.format_table(t, C.UNITS[var]).splitlines()
        assert len(text) == 3 and 'n_valid' in text[0] and text[0].count('[%s]' % C.UNITS[var]) == 3
        assert text[1].split() == ['100000.0', '0', 'nan', 'nan', 'nan']
        assert text[2].split() == ['30000.0', '4', '0.5', '0.8660254', '1.25']
    assert C.UNITS == dict(ta='K', hur='%', ua='m s-1', va='m s-1') and C.VARS == ('ta', 'hur', 'ua', 'va')


# ---- command line and file names -----------------------------------------------------------------------------------------
def test_command_line_and_file_name_rule():
    from pgw4era5_amd import check_deltas as C, settings as S
    args = C.parse_args(['-i', 'in', '-g', 'pgw', '-d', 'deltas', '-o', 'chk', '-f', '2006080200', '-l', '2006080206', '-H', '3'])
    assert args.delta_grid is None
    jobs = C.file_jobs(args)
    assert [j['era_step_dt'] for j in jobs] == [dt.datetime(2006, 8, 2, h) for h in (0, 3, 6)]
    name = S.era5_file_name_base.format(dt.datetime(2006, 8, 2, 3))
    assert jobs[1] == dict(inp_era_file_path=os.path.join('in', name), pgw_era_file_path=os.path.join('pgw', name),
                           delta_input_dir='deltas', era_step_dt=dt.datetime(2006, 8, 2, 3),
                           out_path=os.path.join('chk', 'deltacheck_' + name))
    assert C.check_path('x', '/a/b/' + name) == os.path.join('x', 'deltacheck_' + name)
    for missing in ('-i', '-g', '-d', '-o'):
        argv = [a for f in ('-i', '-g', '-d', '-o') if f != missing for a in (f, 'dir')]
        with pytest.raises(ValueError, match=r'\(%s\) is required' % missing):
            C.parse_args(argv)
    assert C.parse_args(['-i', 'a', '-g', 'b', '-d', 'c', '-o', 'd', '--delta_grid', 'source']).delta_grid == 'source'
    with pytest.raises(SystemExit):
        C.parse_args(['--bands'])                                                                # not built
    with pytest.raises(SystemExit):
        C.parse_args(['-i', 'a', '-g', 'b', '-d', 'c', '-o', 'd', '--delta_grid', 'gcm'])


# ---- errors before any pgw_* call ----------------------------------------------------------------------------------------
def _good(nlev=3, nlat=2, nlon=2):
    from pgw4era5_amd import synthetic
    ak, bk = synthetic.hybrid_coefficients(nlev)
    s3, s4 = (1, nlat, nlon), (1, nlev, nlat, nlon)
    return dict(ps=np.full(s3, 1e5), ta=np.full(s4, 280.0), hus=np.zeros(s4), ua=np.ones(s4), va=np.ones(s4), ak=ak, bk=bk,
                plev=np.array([85000.0, 50000.0]))


BAD = {
    'plev_nan': dict(plev=[85000.0, np.nan]),
    'plev_inf': dict(plev=[np.inf]),
    'plev_small': dict(plev=[85000.0, 0.0001]),
    'plev_negative': dict(plev=[-5.0]),
    'plev_empty': dict(plev=[]),
    'plev_2d': dict(plev=np.ones((2, 2))),
    'plev_too_many': dict(plev=np.linspace(1e3, 1e5, 129)),
    'ak_bk_lengths': dict(bk=np.zeros(5)),
    'level_count': dict(ta=np.full((1, 4, 2, 2), 280.0), hus=np.zeros((1, 4, 2, 2)), ua=np.zeros((1, 4, 2, 2)), va=np.zeros((1, 4, 2, 2))),
    'hus_shape': dict(hus=np.zeros((1, 3, 2, 3))),
    'ua_shape': dict(ua=np.zeros((1, 2, 2, 2))),
    'va_rank': dict(va=np.zeros((3, 2, 2))),
    'ps_grid': dict(ps=np.full((1, 2, 3), 1e5)),
    'ps_rank': dict(ps=np.full((2, 2), 1e5)),
}


@pytest.fixture
def recorder(monkeypatch):
    from pgw4era5_amd import functions as F
    ctx = RecordingContext()
    monkeypatch.setattr(F, 'default_context', lambda: ctx)
    return ctx


@pytest.mark.parametrize('name', sorted(BAD))
def test_argument_errors_make_no_library_call(recorder, name):
    from pgw4era5_amd import functions as F
    a = dict(_good(), **BAD[name])
    one = (a['ps'], a['ta'], a['hus'], a['ua'], a['va'])
    with pytest.raises(ValueError):
        F.state_on_plev(*one, a['ak'], a['bk'], a['plev'])
    with pytest.raises(ValueError):
        F.state_change_on_plev(*one, *one, a['ak'], a['bk'], a['plev'])
    assert recorder.calls == [] and recorder.uploads == []


def test_two_state_argument_errors_make_no_library_call(recorder):
    from pgw4era5_amd import functions as F
    g = _good()
    one = (g['ps'], g['ta'], g['hus'], g['ua'], g['va'])
    rec4, rec3 = np.zeros((1, 2, 2, 2)), np.zeros((1, 2, 2))
    good = dict({v: (rec4, rec4, 5.0, 1.0) for v in K.VARS}, ps_hist=(rec3, rec3, 5.0, 1.0))
    other = np.full((1, 4, 2, 2), 280.0)
    with pytest.raises(ValueError, match='state b'):
        F.state_change_on_plev(*one, g['ps'], other, other, other, other, g['ak'], g['bk'], g['plev'])
    with pytest.raises(ValueError, match='ps_hist is missing'):
        F.state_change_on_plev(*one, *one, g['ak'], g['bk'], g['plev'], deltas={v: good[v] for v in K.VARS})
    with pytest.raises(ValueError, match='records of hur'):
        F.state_change_on_plev(*one, *one, g['ak'], g['bk'], g['plev'], deltas=dict(good, hur=(np.zeros((1, 3, 2, 2)), rec4, 5.0, 1.0)))
    with pytest.raises(ValueError, match='records of ua'):
        F.state_change_on_plev(*one, *one, g['ak'], g['bk'], g['plev'], deltas=dict(good, ua=(rec4, None, 0.0, 0.0)))
    with pytest.raises(ValueError, match='records of ps_hist'):
        F.state_change_on_plev(*one, *one, g['ak'], g['bk'], g['plev'], deltas=dict(good, ps_hist=(rec4, rec4, 5.0, 1.0)))
    assert recorder.calls == [] and recorder.uploads == []
    # ... and a good call is ONE library call with the pointers in the documented order
    change, error = F.state_change_on_plev(*one, *one, g['ak'], g['bk'], g['plev'], deltas=good)
    assert recorder.entries() == ['pgw_state_on_plev']
    assert change.shape == error.shape == (4, 1, 2, 2, 2) and change.dtype == np.float64
    args = recorder.calls[0][1]
    assert args[1:7] == (1, 1, 1, 1, 2, 4) and args[18] == 1                    # float64 tags, ntime, nplev, ncol; dtype_delta
    only, none = F.state_change_on_plev(*one, *one, g['ak'], g['bk'], g['plev'])
    assert none is None and recorder.calls[1][1][-1] is None
    x = F.state_on_plev(*one, g['ak'], g['bk'], g['plev'])
    assert x.shape == (4, 1, 2, 2, 2) and recorder.calls[2][1][13:18] == (None,) * 5


# ---- declaration and binding ---------------------------------------------------------------------------------------------
def test_entry_is_declared_and_bound():
    from pgw4era5_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    m = re.search(r'int pgw_state_on_plev\((.*?)\);', header, re.S)
    assert m, 'pgw_state_on_plev is not declared in include/pgw_hip.h'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, argtypes = _lib.SIGNATURES['pgw_state_on_plev']
    assert len(params) == len(argtypes) == 27 and res is _lib._i
    assert params[7] == 'const double *plev' and params[-1] == 'double *out_error'
    assert re.search(r'PGW_K_COUNT = 28\b', header) and len(_lib.KERNEL_IDS) == 28
    assert 'hybrid_to_plev' in _lib.KERNEL_IDS
