"""CPU tests of the hydrostatic check (pgw4era5_amd/check_geopot.py): the numpy statement the GPU tests compare with
(tests/geopot_statement.py) against hand values and against the oracle's loop, the command line and file-name rule, the
errors raised before any device call, and the table formatting."""
import datetime as dt
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geopot_statement as G                                                         # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from pgw4era5_amd import synthetic                                                   # noqa: E402


# ---- the statement ------------------------------------------------------------------------------------------------------
def test_isothermal_dry_column_by_hand():
    """phi(p) = FIS + Rd T ln(ps / p) wherever p <= ps, for any layering; NaN above ps.  The statement sums Rd T dlnp over
    the layers below k* and adds the partial layer: the sum telescopes, so the bound is a few roundings of a value of
    1e5 m2/s2 (rtol 1e-13)."""
    ak, bk = synthetic.hybrid_coefficients(12)
    ps = np.array([[[101325.0, 90000.0, 60000.0]]])
    fis = np.array([[[0.0, 1500.0, 40000.0]]])
    T = np.full((1, 12, 1, 3), 250.0)
    q = np.zeros_like(T)
    plev = synthetic.PLEV19
    phi = G.phi_on_plev(ps, fis, T, q, ak, bk, plev)
    with np.errstate(invalid='ignore'):
        want = fis[:, None] + O.CON_RD * 250.0 * np.log(ps[:, None] / plev[None, :, None, None])
    below = plev[None, :, None, None] > ps[:, None]
    assert np.array_equal(np.isnan(phi), below)
    np.testing.assert_allclose(phi[~below], want[~below], rtol=1e-13)


def test_edge_columns_of_the_statement():
    e = G.edge_case()
    phi = G.phi_on_plev(e['ps'], e['fis'], e['ta'], e['hus'], e['ak'], e['bk'], e['plev'])[0, :, 0, :]
    col = {n: i for i, n in enumerate(e['names'])}
    lev = {p: i for i, p in enumerate(e['plev'])}
    fis = e['fis'][0, 0]
    assert phi[lev[100000.0], col['ps_on_100000']] == fis[col['ps_on_100000']] == 1234.5       # PS on a level: FIS exactly
    assert phi[lev[85000.0], col['ps_on_85000']] == fis[col['ps_on_85000']]
    assert np.isnan(phi[lev[100000.0], col['ulp_below_100000']]) and np.isfinite(phi[lev[92500.0], col['ulp_below_100000']])
    assert np.isfinite(phi[lev[100000.0], col['ulp_above_100000']])
    assert np.isnan(phi[:19, col['ps_2000']]).sum() == 9                                       # 9 of the 19 CMIP levels
    pa = e['ak'] + 2000.0 * e['bk']
    assert not np.all(np.diff(pa) > 0)                                                         # the column does not ascend
    assert np.isnan(phi[:, col['ps_nan']]).all()
    # the tie level is the pressure of half level k in every column: phi_hl[k] itself, the last term vanishes
    p_tie, k = G.tie_level(e['ak'], e['bk'])
    ps64 = np.asarray(e['ps'], dtype=np.float64)
    pa_hl = e['ak'][None, :, None, None] + ps64[:, None] * e['bk'][None, :, None, None]
    assert np.all(pa_hl[0, k, 0, :6] == p_tie)
    just_above = G.phi_on_plev(e['ps'], e['fis'], e['ta'], e['hus'], e['ak'], e['bk'], [np.nextafter(p_tie, 0.0)])[0, 0, 0]
    np.testing.assert_allclose(phi[lev[p_tie], :5], just_above[:5], rtol=1e-12)                # continuous across the half level


@pytest.mark.parametrize('seed', [0, 5])
def test_error_at_p_ref_is_the_loops_last_max_err(seed):
    """On oracle outputs |phi_error| at p_ref is the loop's last max_err (step_03:298, 308), bit for bit."""
    c = synthetic.make_case(seed=seed)
    era = c['era']
    w = O.pgw_for_era5_arrays(era, c['deltas'], c['delta_times'], c['plev'], c['target_dt'], ignore_top_pressure_error=True)
    zg = O.load_delta_values(c['deltas']['zg'], c['delta_times'], c['target_dt'])[0]
    err = G.phi_error((era['PS'], era['T'], era['QV']), (w['PS'], w['T'], w['QV']), era['FIS'], era['ak'], era['bk'], c['plev'],
                      zg, None, 0.0, 0.0)
    k = list(c['plev']).index(float(O.P_REF_INP))
    assert np.nanmax(np.abs(err[0, k])) == w['max_err'][-1]
    assert w['max_err'][-1] <= O.THRESH_PHI_REF_MAX_ERROR
    share = np.isnan(err).mean()
    assert 0.0 < share <= 0.10
    assert not np.isnan(err[0, list(c['plev']).index(50000.0):]).any()                         # no NaN at 500 hPa and above


# ---- command line and file names -----------------------------------------------------------------------------------------
def test_command_line_and_file_name_rule():
    from pgw4era5_amd import check_geopot as C, settings as S
    args = C.parse_args(['-i', 'in', '-g', 'pgw', '-d', 'deltas', '-o', 'chk', '-f', '2006080200', '-l', '2006080206', '-H', '3'])
    jobs = C.file_jobs(args)
    assert [j['era_step_dt'] for j in jobs] == [dt.datetime(2006, 8, 2, h) for h in (0, 3, 6)]   # last step inclusive
    name = S.era5_file_name_base.format(dt.datetime(2006, 8, 2, 3))
    assert jobs[1] == dict(inp_era_file_path=os.path.join('in', name), pgw_era_file_path=os.path.join('pgw', name),
                           delta_input_dir='deltas', era_step_dt=dt.datetime(2006, 8, 2, 3),
                           out_path=os.path.join('chk', 'zgcheck_' + name))
    assert C.check_path('x', '/a/b/' + name) == os.path.join('x', 'zgcheck_' + name)
    for missing in ('-i', '-g', '-d', '-o'):
        argv = [a for f in ('-i', '-g', '-d', '-o') if f != missing for a in (f, 'dir')]
        with pytest.raises(ValueError, match=r'\(%s\) is required' % missing):
            C.parse_args(argv)
    with pytest.raises(SystemExit):
        C.parse_args(['--bands'])                                                                # no such mode here


# ---- errors before any device call ---------------------------------------------------------------------------------------
class _NoDevice:
    """functions.default_context replaced: a call that reaches the device layer fails the test."""

    def __call__(self):
        raise AssertionError('the device was reached')


def _good(nlev=3, nlat=2, nlon=2):
    ak, bk = synthetic.hybrid_coefficients(nlev)
    s3, s4 = (1, nlat, nlon), (1, nlev, nlat, nlon)
    return dict(ps=np.full(s3, 1e5), zgs=np.zeros(s3), ta=np.full(s4, 280.0), hus=np.zeros(s4), ak=ak, bk=bk,
                plev=np.array([85000.0, 50000.0]))


BAD = {
    'plev_nan': dict(plev=[85000.0, np.nan]),
    'plev_inf': dict(plev=[np.inf]),
    'plev_small': dict(plev=[85000.0, 0.0001]),
    'plev_negative': dict(plev=[-5.0]),
    'plev_empty': dict(plev=[]),
    'plev_2d': dict(plev=np.ones((2, 2))),
    'plev_too_many': dict(plev=np.linspace(1e3, 1e5, 65)),
    'ak_bk_lengths': dict(bk=np.zeros(5)),
    'level_count': dict(ta=np.full((1, 4, 2, 2), 280.0), hus=np.zeros((1, 4, 2, 2))),
    'hus_shape': dict(hus=np.zeros((1, 3, 2, 3))),
    'ps_grid': dict(ps=np.full((1, 2, 3), 1e5)),
    'zgs_rank': dict(zgs=np.zeros((2, 2))),
    'ta_rank': dict(ta=np.full((3, 2, 2), 280.0)),
}


@pytest.mark.parametrize('name', sorted(BAD))
def test_argument_errors_come_before_the_device(monkeypatch, name):
    from pgw4era5_amd import functions as F
    monkeypatch.setattr(F, 'default_context', _NoDevice())
    a = dict(_good(), **BAD[name])
    with pytest.raises(ValueError):
        F.geopot_on_plev(a['ps'], a['zgs'], a['ta'], a['hus'], a['ak'], a['bk'], a['plev'])
    with pytest.raises(ValueError):
        F.geopot_change_on_plev(a['ps'], a['ta'], a['hus'], a['ps'], a['ta'], a['hus'], a['zgs'], a['ak'], a['bk'], a['plev'])


def test_two_state_argument_errors(monkeypatch):
    from pgw4era5_amd import functions as F
    monkeypatch.setattr(F, 'default_context', _NoDevice())
    g = _good()
    two = (g['ps'], g['ta'], g['hus'], g['ps'], g['ta'], g['hus'], g['zgs'], g['ak'], g['bk'], g['plev'])
    with pytest.raises(ValueError, match='dzg must be'):
        F.geopot_change_on_plev(*two, dzg=np.zeros((1, 3, 2, 2)))                               # 3 levels for 2 of plev
    with pytest.raises(ValueError, match='record after'):
        F.geopot_change_on_plev(*two, dzg=(np.zeros((1, 2, 2, 2)), None, 5.0, 1.0))
    with pytest.raises(ValueError, match='form'):
        F.geopot_change_on_plev(*two, form=2)
    other = np.full((1, 4, 2, 2), 280.0)
    with pytest.raises(ValueError, match='state b'):
        F.geopot_change_on_plev(g['ps'], g['ta'], g['hus'], g['ps'], other, other, g['zgs'], g['ak'], g['bk'], g['plev'])
    with pytest.raises(ValueError):
        F.level_stats(np.zeros(5))
    with pytest.raises(ValueError):
        F.level_stats(np.zeros((0, 5)))


# ---- the table -----------------------------------------------------------------------------------------------------------
def test_table_from_given_partials():
    from pgw4era5_amd import check_geopot as C
    plev = [100000.0, 30000.0, 100.0]
    t = C.table_from_partials(plev, [0, 4, 2], [0.0, 2.0, -1.0], [0.0, 3.0, 0.5], [0.0, 1.25, 0.5])
    assert t['n_valid'].tolist() == [0, 4, 2]
    assert np.isnan(t['mean'][0]) and np.isnan(t['rms'][0]) and np.isnan(t['max'][0])
    assert t['mean'][1] == 0.5 and t['rms'][1] == np.sqrt(0.75) and t['max'][1] == 1.25
    assert t['mean'][2] == -0.5 and t['rms'][2] == 0.5
    np.testing.assert_array_equal(t['max_m'][1:], t['max'][1:] / 9.80665)
    text = C.format_table(t, p_ref=30000, thresh=0.15).splitlines()
    assert len(text) == 4 and 'n_valid' in text[0] and 'm2/s2' in text[0]
    assert '<- p_ref' in text[2] and '> thresh_phi_ref_max_error = 0.15' in text[2]
    assert '<- p_ref' not in text[1] and '<- p_ref' not in text[3]
    assert text[1].split()[:2] == ['100000.0', '0'] and text[2].split()[:2] == ['30000.0', '4']
    ok = C.format_table(C.table_from_partials([30000.0], [1], [0.1], [0.01], [0.1]), p_ref=30000, thresh=0.15)
    assert '<= thresh_phi_ref_max_error' in ok
