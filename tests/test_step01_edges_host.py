"""CPU checks of tests/step01_edge_cases.py: every case has the property it was built for, on the oracle alone, so that no
test of tests/test_step01_edges_hip.py can pass vacuously - a NaN-ps column of a 'constant' call IS finite in the
reference, every unsorted list DOES take the kernels' restart, every precedence case DOES hold two different errors and the
reference's column order decides between them as the case expects."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step01_edge_cases as E                                                         # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402


def columns(a):
    """(time, lev, lat, lon) -> (lev, flat column) with the columns in (time, lat, lon) order."""
    return np.moveaxis(a.reshape(a.shape[0], a.shape[1], -1), 1, 0).reshape(a.shape[1], -1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------ a. ps
@pytest.mark.parametrize('ncol', [65, 257])
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('coeff', E.COEFFS)
def test_nonfinite_ps_columns_in_the_reference(coeff, dtype, ncol):
    c = E.ps_case(coeff, dtype, ncol)
    S, n_pure = len(c['ap']), c['n_pure']
    assert n_pure == dict(usual=S // 3, none_pure=0, all_pure=S)[coeff]
    kinds = [v for v in c['special'].values()]
    assert any(np.isnan(v) for v in kinds) and np.inf in kinds and -np.inf in kinds and -3.0e4 in kinds
    assert 0 in c['special'] and 63 in c['special'] and 64 in c['special'] and c['ps'].size - 1 in c['special']
    if ncol == 65:
        assert 65 in c['special'] and c['ps'].shape[0] == 2          # the first column of the second time step
    var = columns(c['var']).astype(np.float64)
    healthy = np.array([p not in c['special'] for p in range(var.shape[1])])
    con = columns(E.reference(c, c['targ'], 'constant'))
    assert np.isfinite(con[:, healthy]).all()
    for mode in ('linear', 'nan'):
        w = columns(E.reference(c, c['targ'], mode))
        assert not np.isnan(w[:, healthy]).all()
        for p, v in c['special'].items():
            if not np.isfinite(v):
                assert np.isnan(w[:, p]).all(), (mode, p, v)
    for p, v in c['special'].items():
        if np.isnan(v) or v == -np.inf:                              # every source logarithm is NaN: above range, last level
            assert np.array_equal(bits(con[:, p]), bits(np.full(con.shape[0], var[-1, p])))
        elif v == np.inf and 0 < n_pure < S:                         # ln: NaN on the pure levels, +inf below: a bracket with NaN
            assert np.isnan(con[:, p]).all()
        elif v == np.inf and n_pure == 0:                            # +inf at level 0: below range, first level
            assert np.array_equal(bits(con[:, p]), bits(np.full(con.shape[0], var[0, p])))
        elif v == np.inf:                                            # 0 * inf = NaN on every level
            assert np.array_equal(bits(con[:, p]), bits(np.full(con.shape[0], var[-1, p])))
    if dtype == 'float64':
        for mode in ('linear', 'constant', 'nan'):
            assert same(E.reference(c, c['targ'], mode), E.reference(c, c['targ'], mode, fast=False))


@pytest.mark.parametrize('first', [0, 5])
@pytest.mark.parametrize('coeff', E.COEFFS)
def test_nonfinite_ps_off_raises_at_the_smallest_special_column(coeff, first):
    c = E.ps_case(coeff, 'float64', 65, first)
    targ = E.inside_every(c, c['targ'], skip=c['special'])
    assert len(targ) >= 3
    assert min(c['special']) == first and np.isnan(c['special'][first])
    assert E.first_error(c['source_P'], E.target_field(c, targ), 'off') == (E.OFF_TEXT, first)
    with pytest.raises(ValueError) as e:
        E.reference(c, targ, 'off')
    assert str(e.value) == E.OFF_TEXT


# ------------------------------------------------------------------------------------------------ b. var
@pytest.mark.parametrize('dtype', E.DTYPES)
def test_nan_and_fill_levels_in_the_reference(dtype):
    c = E.var_case(dtype)
    S = len(c['ap'])
    levels = {lev for lev, _ in c['special'].values()}
    assert {0, S - 1, S // 2} <= levels and any(v == E.FILL for _, v in c['special'].values())
    nan_cols = sorted(p for p, (_, v) in c['special'].items() if np.isnan(v))
    fill_cols = [p for p, (_, v) in c['special'].items() if v == E.FILL]
    for mode in ('linear', 'constant'):
        w = columns(E.reference(c, c['targ'], mode))
        assert sorted(np.nonzero(np.isnan(w).any(axis=0))[0]) == nan_cols
        assert not np.isnan(w[:, nan_cols]).all(axis=0).any()       # the other levels of such a column still interpolate
        assert np.isfinite(w[:, fill_cols]).all() and np.abs(w[:, fill_cols]).max() > 1e18
    off = E.inside_every(c, c['targ'])
    assert len(off) >= 3
    assert E.first_error(c['source_P'], E.target_field(c, off), 'off') is None
    assert np.isnan(E.reference(c, off, 'off')).any()


# ------------------------------------------------------------------------------------------------ c. source order
@pytest.mark.parametrize('dtype', E.DTYPES)
def test_equal_levels_take_the_first_in_the_reference(dtype):
    c = E.equal_levels_case(dtype)
    ap, targ = c['ap'], c['targ']
    assert ap[1] == ap[2] and c['b'][1] == c['b'][2] == 0 and targ[c['hit']] == ap[1] and ap[2] < targ[c['between']] < ap[3]
    assert E.first_error(c['source_P'], E.target_field(c, targ), 'off') is None          # every target inside every column
    for mode in E.MODES:
        w = E.reference(c, targ, mode)
        assert np.array_equal(bits(w[:, c['hit']]), bits(c['var'][:, 1])) and np.all(w[:, c['hit']] != c['var'][:, 2])
        lo, hi = np.minimum(c['var'][:, 2], c['var'][:, 3]), np.maximum(c['var'][:, 2], c['var'][:, 3])
        assert np.all((w[:, c['between']] > lo) & (w[:, c['between']] < hi))


@pytest.mark.parametrize('dtype', E.DTYPES)
def test_crossing_levels_in_the_reference(dtype):
    c = E.crossing_case(dtype)
    sp = columns(c['source_P'])
    low = np.array([p in c['special'] for p in range(sp.shape[1])])
    assert np.all(sp[-1] > sp[0])
    assert np.all(sp[5, low] < sp[4, low]) and np.all(np.diff(sp[:, ~low], axis=0) > 0)
    assert low[0] and not low[1] and low[64] and not low[63]
    for x in (36000.0, 40000.0):
        assert np.all((sp[5, low] < x) & (x < sp[4, low]) & (sp[3, low] < x)) and x in c['targ']
    inside = E.inside_every(c, c['targ'])
    assert E.first_error(c['source_P'], E.target_field(c, inside), 'off') is None and len(inside) >= 5
    want = columns(E.reference(c, c['targ'], 'linear'))
    if dtype == 'float64':
        # the first match of 40000 Pa in a low column is level 4: the bracket (3, 4), not (5, 6)
        var, x = columns(c['var']), np.log(40000.0)
        i = int(np.nonzero(c['targ'] == 40000.0)[0][0])
        l3, l4 = np.log(sp[3]), np.log(sp[4])
        first = var[3] + (x - l3) * (var[4] - var[3]) / (l4 - l3)
        l5, l6 = np.log(sp[5]), np.log(sp[6])
        other = var[5] + (x - l5) * (var[6] - var[5]) / (l6 - l5)
        assert np.array_equal(want[i, low], first[low]) and np.all(want[i, low] != other[low])
        for mode in ('linear', 'constant', 'nan'):
            assert same(E.reference(c, c['targ'], mode), E.reference(c, c['targ'], mode, fast=False))


@pytest.mark.parametrize('dtype', E.DTYPES)
def test_zero_ps_descends_in_the_reference(dtype):
    c = E.zero_ps_case(dtype)
    (col, _), = c['special'].items()
    assert columns(c['source_P'])[-1, col] == 0.0
    inside = E.inside_every(c, c['targ'], skip=[col])
    assert len(inside) >= 3
    for mode, targ in (('constant', c['targ']), ('off', inside)):
        assert E.first_error(c['source_P'], E.target_field(c, targ), mode) == (E.SRC_TEXT, col)
        with pytest.raises(ValueError) as e:
            E.reference(c, targ, mode)
        assert str(e.value) == E.SRC_TEXT


# ------------------------------------------------------------------------------------------------ d. target lists
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('name', sorted(E.LISTS))
def test_unsorted_lists_restart_and_stay_finite(name, dtype):
    c = E.list_case(dtype)
    targ = np.array(E.LISTS[name])
    assert E.restarts(targ) >= 1
    if len(targ) > 1:
        assert not targ[-1] < targ[0]
    con = E.reference(c, targ, 'constant')
    assert np.isfinite(con).all()                                    # a NaN target of a 'constant' call: the last level
    nan = np.isnan(targ)
    if nan.any():
        assert np.array_equal(con[:, nan], np.repeat(c['var'][:, -1:].astype(np.float64), nan.sum(), axis=1))
        assert np.isnan(E.reference(c, targ, 'linear')[:, nan]).all()
    lin = E.reference(c, targ, 'linear')
    assert np.isfinite(lin[:, ~nan]).all()                           # in particular every target after the restart
    assert E.first_error(c['source_P'], E.target_field(c, targ), 'constant') is None
    if dtype == 'float64':
        for mode in ('linear', 'constant', 'nan'):
            assert same(E.reference(c, targ, mode), E.reference(c, targ, mode, fast=False))


def test_the_other_lists():
    assert E.restarts(E.SORTED_DUPLICATES) == 0 and len(set(E.SORTED_DUPLICATES)) < len(E.SORTED_DUPLICATES)
    assert 'duplicates' in E.LISTS and len(set(E.LISTS['duplicates'])) < len(E.LISTS['duplicates'])
    assert E.restarts([5000.0, 1000.0]) == 1 and E.restarts([np.nan, 1000.0]) == 2 and E.restarts([1000.0, 1000.0]) == 0
    c = E.list_case('float64')
    targ = np.array(E.DESCENDING_ENDS)
    assert targ[-1] < targ[0]
    assert E.first_error(c['source_P'], E.target_field(c, targ), 'constant') == (E.TARG_TEXT, 0)
    for name in ('nan_middle', 'nan_first'):                         # through the wrapper: sorted, the NaN last
        s = np.sort(np.array(E.LISTS[name]))
        assert np.isnan(s[-1]) and not np.isnan(s[:-1]).any() and E.restarts(s) == 1


# ------------------------------------------------------------------------------------------------ e. capacity
@pytest.mark.parametrize('dtype', E.DTYPES)
def test_capacity_case(dtype):
    c = E.capacity_case(dtype)
    sp = c['source_P']
    assert c['var'].shape == (1, 256, 1, 3) and len(c['targ']) == 256 and np.all(np.diff(c['targ']) > 0)
    assert c['targ'][0] < sp[:, 0].min() and c['targ'][-1] > sp[:, -1].max()
    assert np.isfinite(E.reference(c, c['targ'], 'constant')).all() and len(E.inside_every(c, c['targ'])) > 200


# ------------------------------------------------------------------------------------------------ f. error precedence
def one_column(sp, tp, col):
    s, t = sp.reshape(sp.shape[0], sp.shape[1], -1), tp.reshape(tp.shape[0], tp.shape[1], -1)
    ti, ci = divmod(col, s.shape[2])
    err = E.first_error(s[ti:ti + 1, :, ci:ci + 1, None], t[ti:ti + 1, :, ci:ci + 1, None], 'off')
    return None if err is None else err[0]


@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('which', ['A', 'B', 'C', 'E'])
def test_precedence_cases_in_the_reference(which, dtype):
    c = E.precedence_case(which, dtype)
    sp, tp = c['source_P'], E.target_field(c, c['targ'])
    text, col = c['expect']
    assert E.first_error(sp, tp, 'off') == (text, col)
    with pytest.raises(ValueError) as e:
        O.interp_logp_4d(c['var'].astype(np.float64), sp, tp, 'off', fast=False)
    assert str(e.value) == text
    # the case holds two different errors, in different columns (A, B, C) or in one (E)
    if which == 'E':
        assert one_column(sp, tp, 0) == E.SRC_TEXT and one_column(sp, tp, 1) == E.TARG_TEXT
    else:
        cols = sorted(c['special'])
        assert {one_column(sp, tp, p) for p in cols} == {E.SRC_TEXT, E.OFF_TEXT} and one_column(sp, tp, cols[0]) == text
        assert all(one_column(sp, tp, p) is None for p in range(sp.shape[3]) if p not in cols)
        assert cols == dict(A=[0, 5], B=[0, 5], C=[0, 256])[which]


@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('both_in_one', [False, True])
def test_precedence_case_d_in_the_reference(both_in_one, dtype):
    c, tp, (text, col) = E.precedence_case_d(both_in_one, dtype)
    sp = c['source_P']
    assert E.first_error(sp, tp, 'off') == (text, col)
    with pytest.raises(ValueError) as e:
        O.interp_logp_4d(c['var'].astype(np.float64), sp, tp, 'off', fast=False)
    assert str(e.value) == text
    if both_in_one:
        assert tp.reshape(tp.shape[1], -1)[-1, 1] < tp.reshape(tp.shape[1], -1)[0, 1] and sp.reshape(sp.shape[1], -1)[-1, 1] < 2000.0
    else:
        assert one_column(sp, tp, 1) == E.OFF_TEXT and one_column(sp, tp, 2) == E.TARG_TEXT and one_column(sp, tp, 0) is None


# ------------------------------------------------------------------------------------------------ Magnus
@pytest.mark.parametrize('dtype', E.DTYPES)
def test_magnus_case(dtype):
    m = E.magnus_case(dtype)
    a, e, want, T, QV, names = m['a'], m['e'], m['want'], m['T'], m['QV'], m['names']
    assert T.dtype == QV.dtype == np.dtype(dtype) and want.dtype == np.float64 and want.shape == T.shape
    aw = a[0, 0, 0, m['window']]
    lo, hi = E.A_WINDOW[dtype]
    sel = E.A_SELECT[dtype]
    assert np.all((aw >= lo) & (aw <= hi)) and np.sum(aw > sel) >= 10 and np.sum(aw <= sel) >= 10
    assert np.all(np.isfinite(want[..., m['window']]) & (want[..., m['window']] > 0))
    tiny = np.finfo(np.dtype(dtype)).tiny
    assert np.all(e[..., m['window']] >= tiny)
    col = lambda k: (slice(None), slice(None), slice(None), names[k])
    assert np.all(np.isinf(e[col('overflow_25K')])) and np.all(want[col('overflow_25K')] == 0)
    if dtype == 'float32':
        assert np.all(np.isinf(e[col('overflow_20K')])) and np.all(want[col('overflow_20K')] == 0)
    else:
        assert np.all(np.isfinite(e[col('overflow_20K')])) and np.all(want[col('overflow_20K')][:, :, 0] > 0)
    for k in ('pole', 'underflow_30K') + (('underflow_40K',) if dtype == 'float32' else ()):
        assert np.all(e[col(k)] == 0)
        assert np.all(np.isposinf(want[col(k)][:, :, 0])) and np.all(np.isnan(want[col(k)][:, :, 1]))     # QV > 0; QV == 0
    assert np.all(T[col('pole')] == np.dtype(dtype).type(29.65)) and np.all(np.isneginf(a[col('pole')]))
    assert np.all(np.isnan(want[col('nan_T')])) and np.all(np.isnan(want[col('plain_200K')][:, :, 1]))
    assert np.all(np.isfinite(want[col('fill_T')])) and np.all(want[col('fill_T')][:, :, 0] > 0)
    assert np.all(want[col('plain_250K')][:, :, 1] > 1e15) and np.all(np.isfinite(want[col('plain_250K')]))
    assert np.all(want[col('plain_300K')][:, :, 1] == 0)
    # every level takes its own pressure
    r = want[0, :, 0, names['plain_320K']] / QV[0, :, 0, names['plain_320K']].astype(np.float64)
    np.testing.assert_allclose(r / r[0], E.MAGNUS_P / E.MAGNUS_P[0], rtol=1e-6)
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0).any()
