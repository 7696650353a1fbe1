"""CPU checks of the cases of tests/wide_plev_cases.py: what the GPU tests of the wide plev table (test_wide_plev_hip.py)
and of zg on its own axis (test_zg_axis_hip.py) rely on is asserted here, so that a later change of `synthetic` cannot
empty them silently - and the Python-side limits, which need no library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_plev_cases as W                                                           # noqa: E402
import local_pref_cases as L                                                          # noqa: E402
from pgw4era5_amd import _lib, synthetic                                              # noqa: E402

# targets whose bracket reaches a source index >= 64 (ascending order): (S, shape) -> count, of 336 / 2280 targets
WIDE_TARGETS = {(65, (3, 7, 16)): 1, (99, (3, 7, 16)): 59, (128, (3, 7, 16)): 189,
                (65, (5, 19, 24)): 56, (99, (5, 19, 24)): 444, (128, (5, 19, 24)): 1425}


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_axes():
    assert len(W.axis(99)) == 99 and W.axis(99)[0] == 101000.0
    for S in (64, 65, 128):
        p = W.axis(S)
        assert len(p) == S and p[0] == 101000.0 and 115.0 <= p[-1] <= 120.0
    assert W.axis(99, top=0.4)[-1] == pytest.approx(0.4) and W.axis(99, top=0.4)[-1] < 0.5      # above the synthetic model top
    for S in (64,) + W.WIDE:
        assert np.sum(W.axis(S) == W.P_REF) == 1


@pytest.mark.parametrize('shape', W.SHAPES, ids=_id)
@pytest.mark.parametrize('S', W.WIDE)
def test_targets_fall_on_both_sides_of_index_64(S, shape):
    f = W.column_facts(W.build(shape, S, 'float64'))
    wide = int(np.sum(f['upper'] >= 64))
    print('S', S, 'shape', shape, 'targets with a bracket index >= 64:', wide, 'of', f['upper'].size)
    assert wide == WIDE_TARGETS[(S, shape)]
    assert 0 < wide < f['upper'].size


def test_the_narrow_boundary_case_stays_narrow():
    for shape in W.SHAPES:
        f = W.column_facts(W.build(shape, 64, 'float64'))
        assert f['upper'].max() <= 64 and f['ksfc'].max() <= 63


@pytest.mark.parametrize('shape,above', [((3, 7, 16), 9), ((5, 19, 24), 33)], ids=_id)
def test_surface_level_of_the_99_level_case(shape, above):
    f = W.column_facts(W.build(shape, 99, 'float64'))
    assert f['ksfc'].min() >= 64                          # every column inserts the surface beyond the narrow table
    assert int(np.sum(f['ps_hist_above'])) == above       # ps_hist > max(plev): the top branch of replace_delta_sfc
    assert np.sum(~f['ps_hist_above']) > 0


@pytest.mark.parametrize('shape', W.SHAPES, ids=_id)
@pytest.mark.parametrize('S', W.WIDE)
def test_oracle_converges_in_six_passes(S, shape):
    assert W.oracle_file(shape, S, 'f64')['n_iter'] == 6


def test_zg_case_levels_lie_on_zg_axis():
    """The loop on zg's own axis: 4 passes, reference levels 50000 to 92500 Pa, all of them levels of PLEV19 and some of
    them no level of the 99-level axis - an implementation that searched the deltas' axis would choose otherwise."""
    shape = W.SHAPES[0]
    c = W.zg_case(shape, 'float64')
    assert c['deltas']['zg'].shape[1] == 19 and c['deltas']['ta'].shape[1] == 99 and len(c['plev']) == 99
    res = W.zg_oracle(shape, 'f64')
    p_ref = np.unique(res['p_ref'])
    print('n_iter', res['n_iter'], 'levels', p_ref)
    assert res['n_iter'] == 4
    assert p_ref.min() == 50000.0 and p_ref.max() == 92500.0
    assert np.all(np.isin(p_ref, synthetic.PLEV19))
    assert not np.all(np.isin(p_ref, c['plev']))
    for t in res['trace']:
        assert t['idx'].min() >= 0 and t['idx'].max() < 19
        assert np.array_equal(synthetic.PLEV19[t['idx']], t['p_ref'])


@pytest.mark.parametrize('dtype', L.DTYPES)
@pytest.mark.parametrize('shape', L.SHAPES, ids=_id)
def test_padding_levels_are_never_chosen(shape, dtype):
    """local_pref_cases.build with two levels appended to zg's axis: the oracle's loop gives the same bits with and
    without them, and the level still moves and is held."""
    from oracle import pgw_oracle as O
    c = L.build(shape, dtype)
    p = W.padded(c)
    assert len(p['plev_zg']) == len(c['plev']) + 2 and p['deltas']['zg'].shape[1] == len(p['plev_zg'])
    i = L.loop_inputs(shape, dtype)
    want, trace = L.oracle_run(shape, dtype, 0.95)
    zg = np.concatenate([i['zg'], np.zeros((i['zg'].shape[0], 2) + i['zg'].shape[2:])], axis=1)
    got = O.adjust_ps_loop_local_pref(i['ak'], i['bk'], i['akm'], i['bkm'], i['PS'], i['FIS'], i['T'], i['QV'], i['ta'], i['hur'],
                                      zg, p['plev_zg'], adj_factor=0.95)
    assert got['n_iter'] == want['n_iter'] and got['max_err'] == want['max_err']
    np.testing.assert_array_equal(got['ps_pgw'], want['ps_pgw'])
    ev = L.events(trace, c['plev'])
    assert sum(ev['changes']) > 0 and sum(ev['clamps']) > 0


# ---------------------------------------------------------------------------------------- limits, without the library
def test_python_side_limits():
    assert _lib.MAX_PLEV == 128 and _lib.MAX_PLEV_ZG == 64
    for n in (2, 64, 65, 99, 128):
        _lib.check_nplev(n)
    _lib.check_nplev(1, 1)
    for n, lo in ((129, 2), (1, 2), (0, 1), (129, 1)):
        with pytest.raises(ValueError, match=r'\[%d, 128\]' % lo):
            _lib.check_nplev(n, lo)
    _lib.check_nplev_zg(1)
    _lib.check_nplev_zg(64)
    for n in (0, 65):
        with pytest.raises(ValueError, match='1 to 64 levels'):
            _lib.check_nplev_zg(n)
