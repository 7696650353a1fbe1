"""GPU tests of the delta check: `pgw_state_on_plev` (k_state_plev) through functions.state_on_plev /
state_change_on_plev, and check_deltas.check_file with its command line, against the numpy statement of
tests/delta_check_cases.py (checked on the CPU by tests/test_delta_check_host.py).

Bounds.  Against the statement: the project's 1e-9 (the kernel's table logarithm against numpy's) - rtol 1e-9 plus atol
1e-9 x the field's max |value|, because winds cross zero inside a bracket.  NaN masks: equal.  What is arithmetic on the
same values in the same order - the fused launch against the composed entries, level orders against each other, two states
against the subtraction of two one-state results, the error against `pgw_time_lerp` of the record pair - is asserted bit
for bit (every NaN counting as one pattern)."""
import ctypes as C
import datetime as dt
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_check_cases as K                                                        # noqa: E402
import points_file_cases as P                                                        # noqa: E402
import source_delta_cases as SD                                                      # noqa: E402
from pgw4era5_amd import synthetic                                                   # noqa: E402

pytestmark = pytest.mark.gpu

RT = 1e-9
LERP, RECORD = dt.datetime(2006, 8, 2, 3), dt.datetime(2006, 8, 15, 12)      # between two monthly records; ON the eighth
F64 = np.dtype('float64')


@pytest.fixture(scope='module')
def F():
    from pgw4era5_amd import functions
    return functions


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    return default_context()


def bits(x):
    """The bit patterns of x with every NaN as one pattern (sign and payload of a NaN are not data)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.where(np.isnan(x), np.uint64(0x7ff8000000000000), x.view(np.uint64))


def close(got, want, what=''):
    """NaN masks equal; values at 1e-9 relative plus 1e-9 of each variable's largest magnitude."""
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    for i, v in enumerate(K.VARS):
        if np.isfinite(want[i]).any():
            scale = np.nanmax(np.abs(want[i]))
            err = np.nanmax(np.abs(got[i] - want[i]) - RT * np.abs(want[i]))
            print('%s %s: max excess over rtol %.3e (atol %.3e)' % (what, v, err, RT * scale))
            np.testing.assert_allclose(got[i], want[i], rtol=RT, atol=RT * scale, equal_nan=True, err_msg='%s %s' % (what, v))


@functools.lru_cache(maxsize=None)
def statement(ncol, nlev, dtype):
    """The statement of state a on PLEV19 (descending), read-only, shared by the tests."""
    c = K.case(ncol, nlev, dtype)
    x = K.state_on_plev(*K.fields(c['era']), c['era']['ak'], c['era']['bk'], K.PLEV19)
    x.setflags(write=False)
    return x


def one_state(F, st, ak, bk, plev):
    return F.state_on_plev(*K.fields(st), ak, bk, plev).numpy()


def composed(ctx, st, ak, bk, plev_sorted):
    """pgw_specific_to_relative_humidity_hybrid + four pgw_interp_hybrid_to_plev (F64 -> F64, PGW_EXTRAP_NAN, ascending list)
    on the arrays widened on the host."""
    from pgw4era5_amd import _lib
    ctx.set_levels(np.asarray(ak, dtype=F64), np.asarray(bk, dtype=F64))
    N = len(ak) - 1
    akm, bkm = (C.c_double * N)(), (C.c_double * N)()
    ctx._check(ctx.lib.pgw_get_full_level_coeffs(ctx.handle, akm, bkm))
    ps, ta, hus, ua, va = (ctx.to_device(np.ascontiguousarray(x, dtype=F64), F64) for x in K.fields(st))
    nt, _, h0, h1 = ta.shape
    ncol, S = h0 * h1, len(plev_sorted)
    rh = ctx.empty(ta.shape, F64)
    ctx._check(ctx.lib.pgw_specific_to_relative_humidity_hybrid(ctx.handle, _lib.PGW_F64, nt, ncol, hus.ptr, ps.ptr, ta.ptr, rh.ptr))
    out = ctx.empty((4, nt, S, h0, h1), F64)
    p = np.ascontiguousarray(plev_sorted, dtype=F64)
    for i, x in enumerate((ta, rh, ua, va)):
        ctx._check(ctx.lib.pgw_interp_hybrid_to_plev(ctx.handle, _lib.PGW_F64, _lib.PGW_F64, nt, N, S, ncol, x.ptr, ps.ptr, akm, bkm,
                                                     p.ctypes.data_as(_lib._dp), _lib.EXTRAP['nan'], 0, 0, out.slab(i).ptr))
    res = out.numpy()
    for d in (ps, ta, hus, ua, va, rh, out):
        d.free()
    return res


# ---- 1. one state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('nlev', K.NLEVS)
@pytest.mark.parametrize('ncol', sorted(K.GRIDS))
def test_one_state_against_the_statement(F, ncol, nlev, dtype):
    c = K.case(ncol, nlev, dtype)
    era = c['era']
    full = statement(ncol, nlev, dtype)
    for S in (1, 5, 19):
        plev = K.level_list(S)
        rows = [list(K.PLEV19).index(p) for p in plev]
        got = one_state(F, era, era['ak'], era['bk'], plev)
        assert got.shape == (4, 1, S) + K.GRIDS[ncol]
        close(got, full[:, :, rows], '%s ncol=%d N=%d S=%d' % (dtype, ncol, nlev, S))
    if nlev == 21 and ncol > 1:
        assert np.isnan(got).mean() <= 0.15                        # a kernel cannot pass by returning NaN


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('ncol,nlev', [(1, 2), (66, 12), (96, 21), (300, 21), (300, 2)])
def test_fused_is_the_composed_calls_bit_for_bit(F, ctx, ncol, nlev, dtype):
    era = K.case(ncol, nlev, dtype)['era']
    for S in (1, 5, 19):
        plev = np.sort(K.level_list(S))
        got = one_state(F, era, era['ak'], era['bk'], plev)
        want = composed(ctx, era, era['ak'], era['bk'], plev)
        assert np.isfinite(want).any() or nlev == 2
        assert np.array_equal(bits(got), bits(want)), (ncol, nlev, dtype, S)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_level_lists_and_orders(F, ctx, dtype):
    """S = 1, 2, 19, 99, 128; ascending, descending, shuffled and repeated levels give the rows of the sorted list, same bits."""
    era = K.case(300, 21, dtype)['era']
    ak, bk = era['ak'], era['bk']
    long = np.unique(np.concatenate([K.PLEV19, np.geomspace(150.0, 99000.0, 128)]))[:128]      # ascending, PLEV19's exact hits among them
    assert long.size == 128
    full = one_state(F, era, ak, bk, long)
    assert np.array_equal(bits(full), bits(composed(ctx, era, ak, bk, long)))
    assert np.isfinite(full).mean() > 0.5
    rng = np.random.default_rng(1)
    orders = dict(descending=np.arange(128)[::-1], shuffled=rng.permutation(128), ninety_nine=rng.permutation(128)[:99],
                  nineteen=np.arange(40, 59), two=np.array([77, 12]), one=np.array([64]), one_top=np.array([0]),
                  repeated=np.array([30, 30, 110, 5, 30]))
    for name, idx in orders.items():
        got = one_state(F, era, ak, bk, long[idx])
        assert got.shape[2] == len(idx)
        assert np.array_equal(bits(got), bits(full[:, :, idx])), name


# ---- 2. the edge columns ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('hybrid_top', [False, True])
@pytest.mark.parametrize('ncol', [None, 66, 96])
def test_edge_columns(F, ncol, hybrid_top, dtype):
    from pgw4era5_amd import step_03_apply_to_era as s3
    e = K.edge_case(ncol, np.dtype(dtype), hybrid_top)
    ak, bk, plev = e['ak'], e['bk'], e['plev']
    a, b = K.fields(e['a']), K.fields(e['b'])
    times = {n: e['times'] for n in e['deltas']}
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(e['times'], e['target'])
    pairs = {n: (r[keep[ib]][None], r[keep[ia]][None], x_hi, x_new) for n, r in e['deltas'].items()}
    xa = F.state_on_plev(*a, ak, bk, plev).numpy()
    change, error = (x.numpy() for x in F.state_change_on_plev(*a, *b, ak, bk, plev, deltas=pairs))
    close(xa, K.state_on_plev(*a, ak, bk, plev), 'edge state a')
    close(change, K.state_change(a, b, ak, bk, plev), 'edge change')
    close(error, K.state_error(a, b, ak, bk, plev, e['deltas'], times, e['target']), 'edge error')
    lev = {p: i for i, p in enumerate(plev)}
    xa, change, error = (x[:, 0, :, 0, :] for x in (xa, change, error))
    for first in (0, len(e['names']) - e['n_edge']):                # the edge columns at the start, and again at the end
        col = {n: first + i for i, n in enumerate(K.EDGE_NAMES)}
        if not hybrid_top:                                          # a pure-pressure full level ON a level: X[k] itself, k = 0 too
            for i, f in enumerate(('T', 'U', 'V')):
                v = (0, 2, 3)[i]
                assert xa[v, lev[10000.0], col['plain']] == np.float64(e['a'][f][0, 2, 0, col['plain']])
                assert xa[v, lev[1000.0], col['plain2']] == np.float64(e['a'][f][0, 0, 0, col['plain2']])
            assert np.isnan(xa[:, lev[500.0]]).all()
        else:                                                       # above the top full level in state b alone
            assert np.isfinite(xa[:, lev[500.0], col['low_in_a']]).all() and np.isnan(change[:, lev[500.0], col['low_in_a']]).all()
        assert np.isnan(change[:, lev[85000.0], col['low_in_a']]).all() and np.isfinite(change[:, lev[85000.0], col['plain']]).all()
        assert np.isnan(error[:, lev[50000.0], col['psh_on_level']]).all() and np.isfinite(error[:, lev[40000.0], col['psh_on_level']]).all()
        assert np.isfinite(error[:, lev[50000.0], col['psh_ulp_above']]).all()
        assert np.isnan(error[:, lev[50000.0], col['psh_ulp_below']]).all()
        assert np.isnan(error[:, :, col['psh_nan']]).all() and np.isfinite(change[:, lev[50000.0], col['psh_nan']]).all()
        assert np.isnan(xa[:, :, col['ps_nan']]).all() and np.isnan(change[:, :, col['descending']]).all() == (not hybrid_top)
        u = xa[2, :, col['wind_sign']]
        assert (u[np.isfinite(u)] > 0).any() and (u[np.isfinite(u)] < 0).any()


# ---- 3. two states ----------------------------------------------------------------------------------------------------------
STORAGE = {'f64/f64': ('float64', 'float64', 'float64'), 'f32 ERA + f64 PGW, f32 2-D': ('float32', 'float64', 'float32'),
           'f32/f32': ('float32', 'float32', 'float32')}


def stored(c, storage):
    ta_, tb_, t2_ = (np.dtype(x) for x in STORAGE[storage])
    a = tuple(x.astype(t2_ if i == 0 else ta_) for i, x in enumerate(K.fields(c['era'])))
    b = tuple(x.astype(t2_ if i == 0 else tb_) for i, x in enumerate(K.fields(c['b'])))
    return a, b


@pytest.mark.parametrize('off64', [0, 1])
@pytest.mark.parametrize('storage', sorted(STORAGE))
@pytest.mark.parametrize('ncol,nlev', [(66, 12), (300, 21)])
def test_two_states(F, ctx, ncol, nlev, storage, off64):
    c = K.case(ncol, nlev)
    a, b = stored(c, storage)
    ak, bk, plev = c['era']['ak'], c['era']['bk'], c['plev']
    old = ctx.set_option('force_off64', off64)
    try:
        xa, xb = F.state_on_plev(*a, ak, bk, plev).numpy(), F.state_on_plev(*b, ak, bk, plev).numpy()
        change, none = F.state_change_on_plev(*a, *b, ak, bk, plev)
    finally:
        ctx.set_option('force_off64', old)
    assert none is None
    change = change.numpy()
    assert np.array_equal(bits(change), bits(xb - xa))
    close(change, K.state_change(a, b, ak, bk, plev), '%s ncol=%d' % (storage, ncol))
    assert np.nanmax(np.abs(change[0])) > 1.0                       # state b is another state
    if off64 == 0:
        old = ctx.set_option('force_off64', 1)
        try:
            wide = F.state_on_plev(*a, ak, bk, plev).numpy()
        finally:
            ctx.set_option('force_off64', old)
        assert np.array_equal(bits(wide), bits(xa))                 # both offset widths: the same bits


@pytest.mark.parametrize('rec_dtype', ['float64', 'float32'])
@pytest.mark.parametrize('instant', ['lerp', 'record', 'five axes'])
def test_error_against_records(F, ncol_nlev, instant, rec_dtype):
    from pgw4era5_amd import step_03_apply_to_era as s3
    ncol, nlev = ncol_nlev
    target = RECORD if instant == 'record' else LERP
    c = K.case(ncol, nlev, 'float64', target)
    a, b = K.fields(c['era']), K.fields(c['b'])
    ak, bk, plev = c['era']['ak'], c['era']['bk'], c['plev']
    names = K.VARS + ('ps_hist',)
    times = K.shifted_axes(c['delta_times']) if instant == 'five axes' else {n: c['delta_times'] for n in names}
    deltas = {n: c['deltas'][n].astype(rec_dtype) for n in names}
    pairs, lerped, xs = {}, {}, set()
    for n in names:
        ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(times[n], target)
        rb, ra = deltas[n][keep[ib]][None], deltas[n][keep[ia]][None]
        pairs[n] = (rb, ra, x_hi, x_new)
        xs.add((x_hi, x_new))
        wide_b, wide_a = rb.astype(np.float64), ra.astype(np.float64)                 # float64 arithmetic on the stored values
        lerped[n] = wide_b if x_hi == 0.0 else F.time_lerp(wide_b, wide_a, x_hi, x_new)
    assert len(xs) == (5 if instant == 'five axes' else 1) and (instant == 'record') == (0.0 in {x for x, _ in xs})
    change, error = (x.numpy() for x in F.state_change_on_plev(*a, *b, ak, bk, plev, deltas=pairs))
    plain = F.state_change_on_plev(*a, *b, ak, bk, plev)[0].numpy()
    assert np.array_equal(bits(change), bits(plain))
    above = np.asarray(plev)[None, :, None, None] < lerped['ps_hist'][:, None]
    for i, n in enumerate(K.VARS):
        want = np.where(above, change[i] - lerped[n], np.nan)
        assert np.array_equal(bits(error[i]), bits(want)), n
    close(error, K.state_error(a, b, ak, bk, plev, deltas, times, target), 'error %s %s' % (instant, rec_dtype))
    assert np.isfinite(error).mean() > 0.5


@pytest.fixture(params=[(66, 12), (300, 21)], ids=['66x12', '300x21'])
def ncol_nlev(request):
    return request.param


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_identical_states(F, dtype):
    from pgw4era5_amd import step_03_apply_to_era as s3
    c = K.case(96, 21, dtype, LERP)
    a = K.fields(c['era'])
    ak, bk, plev = c['era']['ak'], c['era']['bk'], c['plev']
    pairs, lerped = {}, {}
    for n in K.VARS + ('ps_hist',):
        ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(c['delta_times'], LERP)
        rb, ra = c['deltas'][n][keep[ib]][None], c['deltas'][n][keep[ia]][None]
        pairs[n] = (rb, ra, x_hi, x_new)
        lerped[n] = F.time_lerp(rb.astype(np.float64), ra.astype(np.float64), x_hi, x_new)
    xa = F.state_on_plev(*a, ak, bk, plev).numpy()
    change, error = (x.numpy() for x in F.state_change_on_plev(*a, *a, ak, bk, plev, deltas=pairs))
    valid = ~np.isnan(xa)
    assert np.array_equal(np.isnan(change), ~valid) and valid.mean() > 0.8
    assert np.all(change[valid].view(np.uint64) == 0)                                  # +0.0, bit for bit
    above = np.broadcast_to(np.asarray(plev)[None, :, None, None] < lerped['ps_hist'][:, None], valid.shape[1:])
    for i, n in enumerate(K.VARS):
        keep_ = valid[i] & above
        assert np.array_equal(np.isnan(error[i]), ~keep_)
        assert np.array_equal(error[i][keep_].view(np.uint64), (0.0 - lerped[n])[keep_].view(np.uint64)), n


# ---- 4. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(F, ctx):
    from pgw4era5_amd import _lib
    c = K.case(66, 12)
    era, nb = c['era'], c['b']
    ak, bk = era['ak'], era['bk']
    S, ncol, GUARD, FILL = 3, 66, 8, -12345.678
    plev_ok = np.array([85000.0, 50000.0, 20000.0])
    ctx.set_levels(ak, bk)
    d = {k: ctx.to_device(np.ascontiguousarray(v), v.dtype) for k, v in zip('PTQUV', K.fields(era))}
    e = {k: ctx.to_device(np.ascontiguousarray(v), v.dtype) for k, v in zip('PTQUV', K.fields(nb))}
    recs = [ctx.to_device(np.zeros((1, S, 6, 11))) for _ in range(8)]
    psh = [ctx.to_device(np.full((1, 6, 11), 101000.0)) for _ in range(2)]
    host = np.full(4 * S * ncol + GUARD, FILL)
    out, err = ctx.to_device(host), ctx.to_device(host)
    x = (C.c_double * 5)(5.0, 5.0, 5.0, 5.0, 5.0)

    def call(dt2=1, dta=1, dtb=1, nplev=S, plev=plev_ok, a=None, b=None, dtd=1, rb=None, ra=None, pb=True, pa=True, error=True, o=None):
        a = [d[k].ptr for k in 'PTQUV'] if a is None else a
        b = [e[k].ptr for k in 'PTQUV'] if b is None else b
        rb = [r.ptr for r in recs[:4]] if rb is None else rb
        ra = [r.ptr for r in recs[4:]] if ra is None else ra
        p = np.ascontiguousarray(plev, dtype=np.float64)
        return ctx.lib.pgw_state_on_plev(ctx.handle, dt2, dta, dtb, 1, nplev, ncol, p.ctypes.data_as(_lib._dp) if p.size else None, *a, *b, dtd,
                                         C.cast((C.c_void_p * 4)(*rb), _lib._vpp), C.cast((C.c_void_p * 4)(*ra), _lib._vpp),
                                         psh[0].ptr if pb else None, psh[1].ptr if pa else None, x, x,
                                         out.ptr if o is None else o, err.ptr if error else None)
    A = [d[k].ptr for k in 'PTQUV']
    B = [e[k].ptr for k in 'PTQUV']
    bad = dict(
        nplev_zero=dict(nplev=0), nplev_129=dict(nplev=129, plev=np.linspace(1e3, 9e4, 129)),
        level_nan=dict(plev=[85000.0, np.nan, 2e4]), level_inf=dict(plev=[np.inf, 5e4, 2e4]), level_small=dict(plev=[85000.0, 1e-4, 2e4]),
        tag_2d=dict(dt2=7), tag_a=dict(dta=-1), tag_b=dict(dtb=2), tag_delta=dict(dtd=5),
        null_T=dict(a=[A[0], None] + A[2:]), null_PS=dict(a=[None] + A[1:]), null_out=dict(o=0),
        some_b=dict(b=[B[0], B[1], None, B[3], B[4]]), only_ps_b=dict(b=[B[0], None, None, None, None]),
        error_one_state=dict(b=[None] * 5), error_rec_missing=dict(ra=[recs[4].ptr, None, recs[6].ptr, recs[7].ptr]),
        error_psh_missing=dict(pa=False), error_rec_before_missing=dict(rb=[None] + [r.ptr for r in recs[1:4]]),
        misaligned_T=dict(a=[A[0], A[1] + 4] + A[2:]), misaligned_out=dict(o=out.ptr + 4),
        misaligned_rec=dict(rb=[recs[0].ptr + 2] + [r.ptr for r in recs[1:4]]),
    )
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for name, kw in bad.items():
            assert call(**kw) == _lib.PGW_ERR_ARG, name
        with pytest.raises(ValueError):
            F.state_on_plev(*K.fields(era), ak, bk, [np.nan])
        ctx.sync()
        assert ctx.profile_get('hybrid_to_plev') == (0, 0.0)
        for buf in (out, err):                                       # outputs untouched, guard words included
            assert np.array_equal(buf.numpy().view(np.uint64), host.view(np.uint64))
        assert call() == _lib.PGW_OK                                 # the same call with nothing wrong: one launch
        ctx.sync()
        assert ctx.profile_get('hybrid_to_plev')[0] == 1
        for buf in (out, err):
            got = buf.numpy()
            assert np.array_equal(got[-GUARD:].view(np.uint64), host[-GUARD:].view(np.uint64)), 'guard words'
            assert not np.any(got[:-GUARD] == FILL)
    finally:
        ctx.profile(False)


# ---- 5. check_file and the command line ---------------------------------------------------------------------------------------
@pytest.fixture
def clean(monkeypatch):
    """No DeltaSet of an earlier test, PGW_DELTA_GRID as found afterwards, quiet drivers."""
    from pgw4era5_amd import settings as S, step_03_apply_to_era as s3
    P.forget(s3)
    monkeypatch.setenv('PGW_DELTA_GRID', '0')
    monkeypatch.delenv('PGW_DELTA_GRID')
    monkeypatch.setattr(S, 'i_debug', -1)
    yield monkeypatch
    P.forget(s3)


def file_records(delta_dir, instant, H):
    """The record pairs of the instant read from the delta files themselves (not through a DeltaSet)."""
    from pgw4era5_amd import ncio, settings as S, step_03_apply_to_era as s3
    pairs = {}
    for n in K.VARS + ('ps_hist',):
        base, var = (S.file_name_bases['HIST'], 'ps') if n == 'ps_hist' else (S.file_name_bases['SCEN-HIST'], n)
        ds = ncio.open_dataset(os.path.join(delta_dir, base.format(var)))
        v = s3._as_grid(np.asarray(ds[var].values), H)
        ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(np.asarray(ds[S.TIME_GCM].values), instant)
        pairs[n] = (v[keep[ib]][None], v[keep[ia]][None], x_hi, x_new)
    return pairs


def compare_with_functions(F, chk_path, era_path, pgw_path, delta_dir, instant, table):
    """The file's fields against the function-level results (bit for bit) and the table against NaN-skipping numpy."""
    from pgw4era5_amd import ncio, step_03_apply_to_era as s3
    ds, era, pgw = (ncio.open_dataset(p, decode_times=False) for p in (chk_path, era_path, pgw_path))
    H = s3.era_layout(era)
    dims = s3.layout_dims(H)

    def state(f):
        return tuple(s3._as_grid(np.ascontiguousarray(f[n].transpose(*dims['d3' if n == 'PS' else 'd4']).values), H)
                     for n in ('PS', 'T', 'QV', 'U', 'V'))
    a, b = state(era), state(pgw)
    plev = np.asarray(ds['plev'].values)
    ak, bk = np.asarray(era['ak'].values, dtype=np.float64), np.asarray(era['bk'].values, dtype=np.float64)
    change, error = (x.numpy() for x in F.state_change_on_plev(*a, *b, ak, bk, plev, deltas=file_records(delta_dir, instant, H)))
    ncol = int(np.prod(a[0].shape))
    for i, v in enumerate(K.VARS):
        for kind, want in (('change', change), ('error', error)):
            f = ds['%s_%s' % (v, kind)]
            assert tuple(f.dims) == ('time', 'plev') + tuple(H) and f.dtype == np.float64
            assert np.array_equal(bits(np.asarray(f.values).reshape(-1)), bits(want[i].reshape(-1))), (v, kind)
        e2 = error[i].reshape(len(plev), ncol)
        ok = ~np.isnan(e2)
        z, n = np.where(ok, e2, 0.0), ok.sum(axis=1)
        t = table[v]
        assert t['n_valid'].tolist() == n.tolist()
        np.testing.assert_array_equal(t['plev'], plev)
        has = n > 0
        nn = np.where(has, n, 1)
        np.testing.assert_allclose(t['mean'][has], (z.sum(axis=1) / nn)[has], rtol=1e-12, atol=1e-12 * np.abs(z).max())
        np.testing.assert_allclose(t['rms'][has], np.sqrt((z * z).sum(axis=1) / nn)[has], rtol=1e-12)
        np.testing.assert_array_equal(t['max'][has], np.abs(z).max(axis=1)[has])
        assert np.isnan(t['mean'][~has]).all() and np.isnan(t['max'][~has]).all()
    return change, error


def test_check_file_and_command_line(F, ctx, clean, tmp_path, capsys):
    from pgw4era5_amd import check_deltas as CD, settings as S, step_02_preproc_deltas as s2, step_03_apply_to_era as s3
    # --- the mesh case: 10 x 10 columns, 20 levels, deltas on PLEV19 from a 12 x 24 source, on step_02's files and on the GCM's
    instant = SD.INSTANTS[0]
    stamp = '{:%Y%m%d%H}'.format(instant)
    gcm = str(tmp_path / 'gcm')
    synthetic.write_gcm_files(gcm, nlat=12, nlon=24, plev=SD.PLEV, seed=5, ocean=(12, 16))
    era_dir = str(tmp_path / 'era')
    era_path = synthetic.write_case_files(SD.era_case(instant, np.float64), era_dir, str(tmp_path / 'unused'))
    regridded = str(tmp_path / 'regridded')
    assert len(s2.main(['regridding', '-i', gcm, '-o', regridded, '-e', era_path])) == 22
    span = ['-f', stamp, '-l', stamp, '-H', '1']
    name = os.path.basename(era_path)
    maxima = {}
    for reinterp in (0, 1):
        clean.setattr(S, 'i_reinterp', reinterp)
        pgw_dir = str(tmp_path / ('pgw%d' % reinterp))
        s3._cli(['-i', era_dir, '-o', pgw_dir, '-d', regridded, '-t'] + span)
        P.forget(s3)
        capsys.readouterr()
        chk = str(tmp_path / ('chk%d' % reinterp))
        tables = CD._cli(['-i', era_dir, '-g', pgw_dir, '-d', regridded, '-o', chk] + span)
        text = capsys.readouterr().out
        assert len(tables) == 1 and all(('%s_error' % v) in text for v in K.VARS)
        assert text.count('n_valid') == 4 and '[K]' in text and '[%]' in text and text.count('[m s-1]') == 6
        P.forget(s3)
        change, error = compare_with_functions(F, os.path.join(chk, 'deltacheck_' + name), era_path, os.path.join(pgw_dir, name),
                                               regridded, instant, tables[0])
        maxima[reinterp] = {v: float(np.nanmax(tables[0][v]['max'])) for v in K.VARS}
        assert np.isfinite(error).mean() > 0.5
        if reinterp == 0:                                           # the same check on the GCM's files: the same bytes
            P.forget(s3)
            chk_src = str(tmp_path / 'chk_source')
            CD._cli(['-i', era_dir, '-g', pgw_dir, '-d', gcm, '-o', chk_src, '--delta_grid', 'source'] + span)
            capsys.readouterr()
            assert 'PGW_DELTA_GRID' not in os.environ
            assert P.same_files(chk, chk_src) == ['deltacheck_' + name]
            P.forget(s3)
    print('max |error| per variable, i_reinterp = 0: %s' % maxima[0])
    print('max |error| per variable, i_reinterp = 1: %s' % maxima[1])
    assert open(os.path.join(str(tmp_path / 'chk0'), 'deltacheck_' + name), 'rb').read() != \
        open(os.path.join(str(tmp_path / 'chk1'), 'deltacheck_' + name), 'rb').read()
    clean.setattr(S, 'i_reinterp', 0)
    # --- 2-D lat / lon and a cell list
    for case_name in ('rotated 7x9', 'cells 65'):
        P.forget(s3)
        t = P.INSTANTS[0]
        era_d, paths, delta_d = P.write_files(tmp_path, case_name, np.float64, case_name.split()[0], instants=[t])
        out_d = str(tmp_path / (case_name.split()[0] + '_pgw'))
        P.run_files(ctx, paths, out_d, delta_d, instants=[t])
        P.forget(s3)
        chk_path = str(tmp_path / (case_name.split()[0] + '_check.nc'))
        pgw_path = os.path.join(out_d, os.path.basename(paths[0]))
        table = CD.check_file(paths[0], pgw_path, delta_d, t, chk_path)
        P.forget(s3)
        change, error = compare_with_functions(F, chk_path, paths[0], pgw_path, delta_d, t, table)
        assert change.shape[2] == 5 and np.isfinite(error).any()
    # --- a PGW file of another grid
    other = synthetic.make_case(nlat=9, nlon=10, nlev=20, seed=0, target_dt=instant)
    bad = synthetic.write_case_files(other, str(tmp_path / 'other'), str(tmp_path / 'other_deltas'))
    with pytest.raises(ValueError, match='another grid'):
        CD.check_file(era_path, bad, regridded, instant, str(tmp_path / 'never.nc'))
    assert not os.path.exists(str(tmp_path / 'never.nc'))
