"""CPU tests of the cases the local-reference-level GPU tests run on (tests/local_pref_cases.py), with the oracle only:
the level of some column really moves after the first pass, min(p, p_ref_last) really holds columns back, the ties are
exact, no crossing is decided by rounding - and five faults a kernel could have (a restatement of the loop with a switch)
either stop the loop from converging or move PS by far more than the GPU tests' tolerances."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_pref_cases as L                                                          # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

CASES = [(s, d) for s in L.SHAPES for d in L.DTYPES]
MIN_MARGIN = 1.0         # [Pa]; the float32 fast mode's delta_ps differs from the oracle's by about 0.1 Pa
MIN_MUTANT_EFFECT = 1e-4    # relative, in PS: about 100 times the loosest PS tolerance of the GPU tests (1e-6)
_report = {}


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _mutant_effect(i, f, m, want):
    """'does not converge', or the largest relative change of PS."""
    try:
        r = L.loop(i, f, m)
    except ValueError as e:
        assert 'did not converge' in str(e)
        return 'does not converge'
    return float(np.max(np.abs(r['ps_pgw'] - want['ps_pgw']) / want['ps_pgw']))


@pytest.mark.parametrize('adj_factor', L.ADJ_FACTORS)
@pytest.mark.parametrize('shape,dtype', CASES, ids=_id)
def test_the_level_moves_and_is_held_after_the_first_pass(shape, dtype, adj_factor):
    c, i = L.build(shape, dtype), L.loop_inputs(shape, dtype)
    res, trace = L.oracle_run(shape, dtype, adj_factor)
    ev = L.events(trace, i['plev'])
    _report[(shape, dtype, adj_factor, 'events')] = 'passes %d  changes %s  held %s  margin %.2f Pa' % (
        ev['passes'], ev['changes'], ev['clamps'], ev['margin'])
    assert res['n_iter'] == ev['passes'] == len(ev['changes']) + 1
    assert ev['changes'][0] >= 1                                       # pass 2
    if adj_factor == 0.5:
        assert sum(ev['changes'][1:]) >= 1                             # some pass >= 3
        assert res['n_iter'] > 8                                       # more than one full launch of the 8-pass kernel
    assert sum(1 for n in ev['clamps'] if n >= 1) >= 2                 # min(p, p_ref_last) engages in two passes or more
    assert ev['margin'] >= MIN_MARGIN
    assert len(np.unique(res['p_ref'])) > 1
    # only engineered columns move, and they sit in both waves of the 95-column case
    moved = np.zeros(res['p_ref'].size, dtype=bool)
    for a, b in zip(trace[:-1], trace[1:]):
        moved |= (a['idx'] != b['idx']).reshape(-1)
    eng = np.array([col for col, _, _ in c['engineered']])
    assert set(np.nonzero(moved)[0]) <= set(eng)
    if moved.size > 64:
        assert moved[:64].any() and moved[64:].any() and (eng < 64).any() and (eng >= 64).any()
    # the level never comes back down, and it is the level of the index
    for a, b in zip(trace[:-1], trace[1:]):
        assert np.all(b['p_ref'] <= a['p_ref'])
    for t in trace:
        np.testing.assert_array_equal(t['p_ref'], i['plev'][t['idx']])


@pytest.mark.parametrize('shape,dtype', CASES, ids=_id)
def test_engineered_and_tie_columns_are_what_they_claim(shape, dtype):
    c, i = L.build(shape, dtype), L.loop_inputs(shape, dtype)
    plev, ps = i['plev'], i['PS'].reshape(-1)                              # the stored PS as float64
    assert c['era']['PS'].dtype == np.dtype(dtype)
    assert i['ak'][-1] == 0.0 and i['bk'][-1] == 1.0                       # the lowest half level IS the surface pressure
    assert len(c['engineered']) == -(-ps.size // 3)
    for col, k, eps in c['engineered']:
        assert col % 3 == 0
        d = 0.95 * ps[col] - plev[k]
        assert abs(d - eps) < 0.02 and d > 1.0                              # (float32 PS: 0.0078 Pa spacing)
        assert not np.any((plev > plev[k]) & (plev < 0.95 * ps[col]))       # plev[k] is the first level above the surface
    kinds = [kind for _, _, kind in c['ties']]
    assert kinds.count('below') == kinds.count('above') >= 2
    assert (kinds.count('exact') >= 2) if dtype == 'float64' else ('exact' not in kinds)
    T = np.dtype(dtype).type
    by_level = {}
    for col, k, kind in c['ties']:
        assert col % 3 == 1
        p = 0.95 * ps[col]
        if kind == 'exact':
            assert p == plev[k]
        elif kind == 'below':
            assert p < plev[k] and 0.95 * np.float64(np.nextafter(T(ps[col]), T(np.inf))) >= plev[k]
        else:
            assert p > plev[k] and 0.95 * np.float64(np.nextafter(T(ps[col]), T(0))) <= plev[k]
        by_level.setdefault(k, set()).add(kind)
    assert all(kk == set(kinds) for kk in by_level.values())                # every tie level has its whole family
    # a tie column's delta_ps stays clearly positive: the PGW state never decides its level, the ERA comparison does
    tcols = [col for col, _, _ in c['ties']]
    for f in L.ADJ_FACTORS:
        res, trace = L.oracle_run(shape, dtype, f)
        for t in trace[1:]:
            assert np.all(t['ps_pgw'].reshape(-1)[tcols] > ps[tcols] + 2.0)
        idx = res['p_ref'].reshape(-1)
        for col, k, kind in c['ties']:
            assert idx[col] == (plev[k] if kind == 'above' else plev[k + 1]), (col, kind)   # `>`: a tie takes the next level


@pytest.mark.parametrize('adj_factor', L.ADJ_FACTORS)
@pytest.mark.parametrize('shape,dtype', CASES, ids=_id)
def test_mutants_of_the_level_rule_are_visible(shape, dtype, adj_factor):
    i = L.loop_inputs(shape, dtype)
    want, _ = L.oracle_run(shape, dtype, adj_factor)
    same = L.loop(i, adj_factor)
    assert same['n_iter'] == want['n_iter'] and same['max_err'] == want['max_err']
    np.testing.assert_array_equal(same['ps_pgw'], want['ps_pgw'])
    np.testing.assert_array_equal(same['hus_pgw'], want['hus_pgw'])
    effects = {}
    for m in L.MUTANTS:
        if m == 'ge' and dtype == 'float32':
            continue                                        # no float32 PS hits a level exactly: nothing for `>=` to change
        effects[m] = e = _mutant_effect(i, adj_factor, m, want)
        assert e == 'does not converge' or e >= MIN_MUTANT_EFFECT, (m, e)
    _report[(shape, dtype, adj_factor, 'mutants')] = '  '.join(
        '%s: %s' % (m, e if isinstance(e, str) else 'PS moves by %.2e' % e) for m, e in effects.items())


def test_error_case_finds_every_level_in_pass_1_and_none_later():
    i = L.loop_inputs()
    trace = []
    with pytest.raises(ValueError, match='No reference pressure level'):
        O.adjust_ps_loop_local_pref(i['ak'], i['bk'], i['akm'], i['bkm'], i['PS'], i['FIS'], i['T'], i['QV'], i['ta'], i['hur'],
                                    i['zg'], i['plev'], trace=trace)
    assert len(trace) >= 2
    for t in trace[:-1]:
        assert np.all(t['idx'] >= 0) and not np.any(np.isnan(t['p_ref']))
    assert trace[0]['p_ref'][0, 0, 0] == 85000.0
    bad = np.isnan(trace[-1]['p_ref'])
    assert bad.sum() == 1 and bad[0, 0, 0] and trace[-1]['idx'][0, 0, 0] == -1
    _report[('error case',)] = 'no level for column 0 in pass %d' % len(trace)


@pytest.mark.parametrize('adj_factor', L.ADJ_FACTORS)
def test_refdtype_oracle_local_rule_on_float64_inputs_is_the_float64_oracle(adj_factor):
    """oracle/pgw_oracle_refdtype.py follows numpy's promotion: on float64 operands its local-level loop (i_reinterp = 0) and
    its whole-file form are the float64 oracle's."""
    shape = L.SHAPES[0]
    c, i = L.build(shape, 'float64'), L.loop_inputs(shape, 'float64')
    want, _ = L.oracle_run(shape, 'float64', adj_factor)
    got = R.adjust_ps_loop_local_pref(i['ak'], i['bk'], i['akm'], i['bkm'], i['PS'], i['FIS'], i['T'], i['QV'], i['ta'], i['hur'],
                                      i['zg'], i['plev'], adj_factor=adj_factor)
    assert got['n_iter'] == want['n_iter'] and got['max_err'] == want['max_err']
    for k in ('ps_pgw', 'hus_pgw', 'p_ref'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    whole = R.pgw_for_era5_arrays(*L.args_of(c), p_ref=None, adj_factor=adj_factor)
    assert whole['n_iter'] == want['n_iter']
    np.testing.assert_allclose(whole['PS'], want['ps_pgw'], rtol=1e-13)
    np.testing.assert_allclose(whole['QV'], want['hus_pgw'], rtol=1e-11, atol=1e-20)


def test_reinterp_oracle_passes_the_adjustment_factor_through():
    c = L.build(L.SHAPES[0], 'float64')
    for pr in (None, 30000.0):
        a = O.pgw_for_era5_arrays_reinterp(*L.args_of(c), p_ref=pr)
        b = O.pgw_for_era5_arrays_reinterp(*L.args_of(c), p_ref=pr, adj_factor=0.5)
        assert b['n_iter'] > a['n_iter']
        np.testing.assert_allclose(b['PS'], a['PS'], rtol=2e-5)         # the same fixed point, approached more slowly


def test_report_the_event_counts_once(capsys):
    """The last test of the module prints, once, what the tests above measured: per case and adjustment factor the passes,
    the level changes and the held columns per pass (from pass 2 on), the smallest crossing margin and each mutant's effect
    on PS."""
    lines = ['', 'local reference level: events per case (oracle trace; lists start at pass 2)']
    for key in sorted(_report, key=str):
        lines.append('  %-28s %s' % (' '.join(_id(v) for v in key), _report[key]))
    with capsys.disabled():
        print('\n'.join(lines))
