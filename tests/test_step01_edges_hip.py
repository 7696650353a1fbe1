"""GPU checks of the step_01 kernels on the cases of tests/step01_edge_cases.py (tests/test_step01_edges_host.py shows on
the CPU that every case has the property it is here for).

k_hybrid_to_plev: columns whose ps is NaN, +-inf or negative beside healthy ones, with some, no and only pure-pressure
levels (the shared logarithms of the pure levels must not serve a column whose 0 * ps is NaN); NaN and fill values in var;
source columns that are legal without ascending strictly; target lists that take the scan's restart (through
step_01_extract_deltas._launch_hybrid, because interp_to_plev sorts its list); the largest level counts and the refusal of
larger ones.  Every comparison covers all cells: the tolerance of tests/test_step01_hip.py with equal_nan, the same NaN
and the same inf positions.  Each case runs on float64 input, on float32 input with float64 output (the reference's dtype
flow) and with float32 output (float64 arithmetic narrowed once: the float64 run on the widened input, narrowed), with
both level orders of the input and of the output.

Both interpolation kernels: which error a call raises when several columns, or one column, hold different ones - the
reference walks the columns in (time, lat, lon) order and checks the source ends, the target ends and then the targets.

k_magnus_rh: both sides of its exp range select, overflow, underflow, the pole of the exponent and missing values,
against numpy's dtype flow."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step01_edge_cases as E                                                         # noqa: E402
from test_step01_hip import ATOL, RTOL                                                # noqa: E402

pytestmark = pytest.mark.gpu

assert (RTOL, ATOL) == (1e-10, 1e-12)
REVS = [(False, False), (True, False), (False, True), (True, True)]
VALUE_MODES = ('linear', 'constant', 'nan')


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    return default_context()


@pytest.fixture(scope='module')
def s1():
    from pgw4era5_amd import step_01_extract_deltas
    return step_01_extract_deltas


def compare(got, want, what=''):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN positions %s' % (what,)
    assert np.array_equal(np.isinf(got), np.isinf(want)), 'inf positions %s' % (what,)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=str(what))


def flipped(case, src_rev):
    sl = slice(None, None, -1) if src_rev else slice(None)
    return np.ascontiguousarray(case['var'][:, sl]), np.ascontiguousarray(case['ap'][sl]), np.ascontiguousarray(case['b'][sl])


def wrapper(s1, case, targ, mode, src_rev=False, out_rev=False, out_dtype=None, widen=False):
    var, ap, b = flipped(case, src_rev)
    ps = case['ps']
    if widen:
        var, ps = var.astype(np.float64), ps.astype(np.float64)
    return s1.interp_to_plev(var, ps, ap, b, targ, extrapolate=mode, lev_descending=src_rev, plev_descending=out_rev,
                             out_dtype=out_dtype)


def launch(ctx, s1, case, targ, mode, src_rev=False, out_rev=False, out_dtype='float64', widen=False):
    """pgw_interp_hybrid_to_plev on the list as it is (interp_to_plev would sort it)."""
    from pgw4era5_amd.operands import check_extrapolate
    var, ap, b = flipped(case, src_rev)
    ps = case['ps']
    if widen:
        var, ps = var.astype(np.float64), ps.astype(np.float64)
    targ = np.ascontiguousarray(targ, dtype=np.float64)
    out = ctx.empty((var.shape[0], max(len(targ), 1)) + var.shape[2:], np.dtype(out_dtype))
    s1._launch_hybrid(ctx, ctx.to_device(var), ctx.to_device(np.ascontiguousarray(ps)), ap, b, targ, check_extrapolate(mode),
                      src_rev, out_rev, out)
    return out.numpy()


def all_forms(run, case, want, what):
    """`run(src_rev, out_rev, out_dtype, widen)` in every level order: the case's dtype with float64 output against `want`;
    float32 input with float32 output against the float64 arithmetic on the widened input, narrowed once."""
    for src_rev, out_rev in REVS:
        w = want[:, ::-1] if out_rev else want
        got = run(src_rev, out_rev, None, False)
        assert got.dtype == np.float64
        compare(got, w, (what, src_rev, out_rev))
        if case['var'].dtype == np.float32:
            got32 = run(src_rev, out_rev, 'float32', False)
            wide = run(src_rev, out_rev, None, True)
            assert got32.dtype == np.float32 and wide.dtype == np.float64
            with np.errstate(over='ignore'):
                assert np.array_equal(got32, wide.astype(np.float32), equal_nan=True), (what, src_rev, out_rev, 'float32 out')


def check_wrapper(s1, case, targ, mode, what=''):
    want = E.reference(case, targ, mode)
    assert want.dtype == np.float64
    all_forms(lambda sr, orv, od, wd: wrapper(s1, case, targ, mode, sr, orv, od, wd), case, want, (what, mode))
    return want


def raises(text, column, fn):
    with pytest.raises(ValueError) as e:
        fn()
    assert str(e.value) == text
    assert e.value.column == column
    return e.value


def healthy_call(s1, dtype='float64'):
    """The context computes after an error."""
    c = E.list_case(dtype, 5)
    compare(wrapper(s1, c, c['targ'], 'linear'), E.reference(c, c['targ'], 'linear'), 'healthy call')


# ------------------------------------------------------------------------------------------------ a. ps
@pytest.mark.parametrize('ncol', [65, 257])
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('coeff', E.COEFFS)
@pytest.mark.parametrize('mode', VALUE_MODES)
def test_nonfinite_and_negative_ps(s1, mode, coeff, dtype, ncol):
    c = E.ps_case(coeff, dtype, ncol)
    check_wrapper(s1, c, c['targ'], mode, coeff)
    if mode == 'constant':
        got = wrapper(s1, c, c['targ'], mode)
        g = got.reshape(got.shape[0], got.shape[1], -1)
        v = c['var'].astype(np.float64).reshape(g.shape[0], -1, g.shape[2])
        for p, val in c['special'].items():
            if np.isnan(val) or val == -np.inf:                     # the highest-pressure level at every target, bit for bit
                t, i = divmod(p, g.shape[2])
                assert np.array_equal(np.ascontiguousarray(g[t, :, i]).view(np.uint64), np.full(g.shape[1], v[t, -1, i]).view(np.uint64)), p
            elif val == np.inf and 0 < c['n_pure'] < len(c['ap']):
                t, i = divmod(p, g.shape[2])
                assert np.isnan(g[t, :, i]).all(), p


@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('first', [0, 5])
@pytest.mark.parametrize('coeff', E.COEFFS)
def test_nonfinite_ps_off_raises_at_the_smallest_column(s1, coeff, first, dtype):
    c = E.ps_case(coeff, dtype, 65, first)
    targ = E.inside_every(c, c['targ'], skip=c['special'])
    for src_rev, out_rev in REVS:
        raises(E.OFF_TEXT, first, lambda: wrapper(s1, c, targ, 'off', src_rev, out_rev))
    healthy_call(s1, dtype)


# ------------------------------------------------------------------------------------------------ b. var
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('mode', E.MODES)
def test_nan_and_fill_values_in_var(s1, mode, dtype):
    c = E.var_case(dtype)
    targ = E.inside_every(c, c['targ']) if mode == 'off' else c['targ']
    want = check_wrapper(s1, c, targ, mode)
    assert np.isnan(want).any()


# ------------------------------------------------------------------------------------------------ c. source order
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('mode', E.MODES)
def test_equal_levels_take_the_first(s1, mode, dtype):
    c = E.equal_levels_case(dtype)
    check_wrapper(s1, c, c['targ'], mode)
    for src_rev in (False, True):
        got = wrapper(s1, c, c['targ'], mode, src_rev)
        assert np.array_equal(got[:, c['hit']].view(np.uint64), c['var'][:, 1].astype(np.float64).view(np.uint64))


@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('mode', E.MODES)
def test_levels_that_cross_for_low_ps_only(s1, mode, dtype):
    c = E.crossing_case(dtype)
    targ = E.inside_every(c, c['targ']) if mode == 'off' else c['targ']
    check_wrapper(s1, c, targ, mode)


@pytest.mark.parametrize('dtype', E.DTYPES)
def test_zero_ps_raises_the_source_text_at_its_column(s1, dtype):
    c = E.zero_ps_case(dtype)
    (col, _), = c['special'].items()
    inside = E.inside_every(c, c['targ'], skip=[col])
    for mode, targ in (('constant', c['targ']), ('off', inside), ('linear', c['targ'])):
        for src_rev, out_rev in REVS:
            raises(E.SRC_TEXT, col, lambda: wrapper(s1, c, targ, mode, src_rev, out_rev))
    healthy_call(s1, dtype)


# ------------------------------------------------------------------------------------------------ d. target lists
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('mode', VALUE_MODES)
@pytest.mark.parametrize('name', sorted(E.LISTS) + ['sorted_duplicates'])
def test_lists_the_wrapper_cannot_produce(ctx, s1, name, mode, dtype):
    c = E.list_case(dtype)
    targ = np.array(E.SORTED_DUPLICATES if name == 'sorted_duplicates' else E.LISTS[name])
    want = E.reference(c, targ, mode)
    all_forms(lambda sr, orv, od, wd: launch(ctx, s1, c, targ, mode, sr, orv, od or 'float64', wd), c, want, (name, mode))


@pytest.mark.parametrize('dtype', E.DTYPES)
def test_descending_list_raises_the_target_text_at_column_0(ctx, s1, dtype):
    c = E.list_case(dtype)
    for mode in ('constant', 'off'):
        raises(E.TARG_TEXT, 0, lambda: launch(ctx, s1, c, E.DESCENDING_ENDS, mode))
    healthy_call(s1, dtype)


@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('mode', VALUE_MODES)
@pytest.mark.parametrize('name', ['nan_middle', 'nan_first'])
def test_the_wrapper_sorts_a_nan_last(s1, name, mode, dtype):
    c = E.list_case(dtype)
    targ = np.array(E.LISTS[name])
    want = E.reference(c, np.sort(targ), mode)
    all_forms(lambda sr, orv, od, wd: wrapper(s1, c, targ, mode, sr, orv, od, wd), c, want, (name, mode))


# ------------------------------------------------------------------------------------------------ e. capacity
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('mode', E.MODES)
def test_256_levels_onto_256_targets(s1, mode, dtype):
    c = E.capacity_case(dtype)
    targ = E.inside_every(c, c['targ']) if mode == 'off' else c['targ']
    check_wrapper(s1, c, targ, mode)


def test_level_counts_out_of_range_are_refused_before_a_launch(ctx, s1):
    from pgw4era5_amd import _lib
    nlat, nlon = 1, 3
    ps = np.full((1, nlat, nlon), 1.0e5)
    targ = np.geomspace(3000.0, 9.0e4, 257)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        for S, N, text in ((257, 5, 'between 2 and 256 model levels are supported, got 257'),
                           (5, 257, 'between 1 and 256 target levels are supported, got 257'),
                           (1, 5, 'between 2 and 256 model levels are supported, got 1'),
                           (5, 0, 'between 1 and 256 target levels are supported, got 0')):
            ap, b = np.linspace(2000.0, 0.0, S), np.linspace(0.0, 1.0, S)
            var = np.full((1, S, nlat, nlon), 250.0)
            with pytest.raises(ValueError) as e:
                s1.interp_to_plev(var, ps, ap, b, targ[:N], lev_descending=False)
            assert str(e.value) == text
            # the C entry itself, on arrays of the size it is told
            out = ctx.empty((1, max(N, 1), nlat, nlon), np.float64)
            with pytest.raises(ValueError) as e:
                s1._launch_hybrid(ctx, ctx.to_device(var), ctx.to_device(ps), ap, b, np.ascontiguousarray(targ[:N]), 2, False, False, out)
            assert e.value.status == _lib.PGW_ERR_ARG
        assert ctx.profile_get('hybrid_to_plev')[0] == 0
    finally:
        ctx.profile(False)
    healthy_call(s1)


# ------------------------------------------------------------------------------------------------ f. error precedence
@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('which', ['A', 'B', 'C'])
def test_precedence_fused_kernel(s1, which, dtype):
    c = E.precedence_case(which, dtype)
    text, col = c['expect']
    for src_rev, out_rev in REVS:
        raises(text, col, lambda: wrapper(s1, c, c['targ'], 'off', src_rev, out_rev))
    healthy_call(s1, dtype)


@pytest.mark.parametrize('dtype', E.DTYPES)
def test_precedence_fused_kernel_source_before_target_list(ctx, s1, dtype):
    c = E.precedence_case('E', dtype)
    text, col = c['expect']
    for mode in ('off', 'constant'):
        raises(text, col, lambda: launch(ctx, s1, c, c['targ'], mode))
    healthy_call(s1, dtype)


@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('which', ['A', 'B', 'C'])
def test_precedence_interp_logp_4d(s1, which, dtype):
    from pgw4era5_amd import functions as F
    c = E.precedence_case(which, dtype)
    text, col = c['expect']
    tp = E.target_field(c, c['targ'])
    raises(text, col, lambda: F.interp_logp_4d(c['var'], c['source_P'], tp, 'off'))
    healthy_call(s1, dtype)


@pytest.mark.parametrize('dtype', E.DTYPES)
@pytest.mark.parametrize('both_in_one', [False, True])
def test_precedence_interp_logp_4d_per_column_targets(s1, both_in_one, dtype):
    from pgw4era5_amd import functions as F
    c, tp, (text, col) = E.precedence_case_d(both_in_one, dtype)
    raises(text, col, lambda: F.interp_logp_4d(c['var'], c['source_P'], tp, 'off'))
    # the healthy columns of the same fields compute afterwards
    sl = (slice(None), slice(None), slice(None), slice(3, None))
    targ_ok = np.ascontiguousarray(tp[sl])
    got = F.interp_logp_4d(np.ascontiguousarray(c['var'][sl]), np.ascontiguousarray(c['source_P'][sl]), targ_ok, 'off')
    mod = E.O if dtype == 'float64' else E.R
    compare(got, mod.interp_logp_4d(c['var'][sl], c['source_P'][sl], targ_ok, 'off'), 'columns 3 ..')


# ------------------------------------------------------------------------------------------------ Magnus
@pytest.mark.parametrize('dtype', E.DTYPES)
def test_magnus_selects_and_missing_values(s1, dtype):
    m = E.magnus_case(dtype)
    got = s1.specific_to_relative_humidity(m['QV'], m['P'], m['T'])
    want = m['want']
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf])
    assert np.array_equal(got == 0, want == 0)
    ok = np.isfinite(want) & (want != 0)
    assert ok.sum() > 200
    dev = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
    a = m['a'][ok]
    worst = int(np.argmax(dev))
    print('\nMagnus %s: largest relative deviation %.3e (%.2f float32 ulp) at exponent %.4f' % (dtype, dev[worst], dev[worst] / 2.0**-23, a[worst]))
    assert dev.max() <= (1e-13 if dtype == 'float64' else 2.4e-7)          # the bounds of tests/test_step01_hip.py
    # a 4-D P that holds the list in every column is the same call
    got4 = s1.specific_to_relative_humidity(m['QV'], np.broadcast_to(m['P'][None, :, None, None], want.shape), m['T'])
    assert np.array_equal(got4, got, equal_nan=True)
