"""PGW_OPT_QV_FROM_PASS ('qv_from_pass'): the last pass of every multi-pass loop launch also stores the QV it forms below
p_ref, and when that pass is the converged one the finalize kernel computes only the levels above each wave's stopping
point.  The option changes who writes a value, never the value: with it on (default) and off, in one process, every output
has the same bits, the loop runs and launches the same passes and records the same max|err| history.  The getter
`Context.last_qv_from_pass()` says which way the last file went, so both the used and the discarded prediction are pinned.

Not covered here: a file split in latitude bands with the option on against one rank with it off - the tests' helpers have
no one-process rehearsal of the reduce hook (tests/test_hip_files.py::_run_bands starts a process group); the band tests of
tests/test_hip_files.py and tests/test_fused_first.py run with the option at its default, on."""
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RECORD = dt.datetime(2006, 3, 15, 12)          # an instant that is a delta record: no time interpolation
STORAGE = {'f64': (np.float64, False), 'f32': (np.float32, False), 'f32ref': (np.float32, True)}
FIELDS = ('PS', 'T', 'QV', 'U', 'V', 'RELHUM_pgw')
# float32 fast mode does not take the path (its loop kernel lost more than its finalize kernel gained: DESIGN.md section 4):
# its instantiation of the loop kernel is the one without the store, and the marks are never used there
TAKES_PATH = {'f64': True, 'f32': False, 'f32ref': True}


def _case(nlat=8, nlon=12, nlev=27, seed=81, dtype=np.float64, **kw):
    from pgw4era5_amd import synthetic
    return synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=seed, dtype=dtype, **kw)


def _both(c, ref_dtype=False, opts=None, **kw):
    """The file with qv_from_pass = 1 and = 0 (other options as given, the same for both; loop_guess is set before each
    run, because every file leaves its own pass count there).  Returns [(result, (used, skipped)), ...]."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    opts = dict(opts or {})
    guess = opts.pop('loop_guess', None)
    old = {k: ctx.set_option(k, v) for k, v in opts.items()}
    old['qv_from_pass'] = ctx.get_option('qv_from_pass')
    old['loop_guess'] = ctx.get_option('loop_guess')
    res = []
    try:
        for on in (1, 0):
            ctx.set_option('qv_from_pass', on)
            if guess is not None:
                ctx.set_option('loop_guess', guess)
            try:
                r = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True,
                                           ref_dtype=ref_dtype, **kw)
            except ValueError as e:
                r = e
            res.append((r, ctx.last_qv_from_pass()))
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
    return res


def _same(a, b):
    assert not isinstance(a, Exception) and not isinstance(b, Exception), (a, b)
    assert a['n_iter'] == b['n_iter']
    np.testing.assert_array_equal(np.asarray(a['max_err']), np.asarray(b['max_err']))
    assert a['passes_launched'] == b['passes_launched']
    for k in FIELDS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _check(res, used):
    """Same file either way; with the option off the marks are never used; with it on they are used exactly when `used`
    (None: not asserted), and then the finalize kernel skipped something."""
    (a, ma), (b, mb) = res
    _same(a, b)
    assert mb == (False, 0)
    if used is not None:
        assert ma[0] == used
    assert (ma[1] > 0) == ma[0]
    return a


def test_option_defaults_to_on():
    from pgw4era5_amd.device import default_context
    assert default_context().get_option('qv_from_pass') == 1


@pytest.mark.parametrize('target', [None, RECORD], ids=['lerp', 'record'])
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_storage_and_instant(storage, target):
    """float64, float32 fast and float32 reference-dtype storage; an instant between two records and one that is a record.
    The surface of synthetic.make_case spans about 1013 - 540 hPa: the waves pass p_ref at different model levels.  The
    first launch is as long as the file's loop (6 passes), so the converged pass stores."""
    dtype, ref = STORAGE[storage]
    c = _case(dtype=dtype, target_dt=target)
    assert c['era']['PS'].min() < 70000.0 < c['era']['PS'].max()
    a = _check(_both(c, ref, dict(loop_guess=6)), TAKES_PATH[storage])
    assert a['n_iter'] == 6


@pytest.mark.parametrize('fused', [1, 0], ids=['fused', 'unfused'])
@pytest.mark.parametrize('guess,used', [(6, True), (2, True), (1, False), (5, False), (8, False)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_prediction_used_and_discarded(storage, guess, used, fused):
    """The file needs 6 passes.  A first launch of 6 passes, or of 2 followed by two continuation launches of 2, ends with
    the converged pass: the marks are used.  With 1 (+2+2+2), 5 (+2) or 8 passes in the first launch the converged pass is
    the first of a continuation launch or inside the first launch: the speculated QV is overwritten by a full finalize."""
    dtype, ref = STORAGE[storage]
    c = _case(dtype=dtype)
    a = _check(_both(c, ref, dict(loop_guess=guess, fused_first=fused)), used and TAKES_PATH[storage])
    assert a['n_iter'] == 6


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_several_blocks_and_a_partial_last_wave(storage):
    """23 x 29 = 667 columns: several blocks, the last wave with 27 of 64 lanes, an odd column count (one column per
    thread in the finalize kernel as well)."""
    dtype, ref = STORAGE[storage]
    c = _case(23, 29, 31, seed=5, dtype=dtype)
    n = _both(c, ref)[0][0]['n_iter']                       # this file's own pass count, then predicted exactly
    _check(_both(c, ref, dict(loop_guess=n)), TAKES_PATH[storage])


def _bend_one_layer(c, ps_turn):
    """Alter ak at one half level so that the layer above it has zero thickness at ps = ps_turn and a negative one below:
    ps_mono_min (the smallest ps with strictly ascending half-level pressures) becomes ps_turn."""
    era = dict(c['era'])
    ak, bk = era['ak'].copy(), era['bk'].copy()
    l = len(ak) - 6
    assert bk[l + 1] > bk[l]
    ak[l + 1] = ak[l] - ps_turn * (bk[l + 1] - bk[l])
    era['ak'] = ak
    era['akm'] = 0.5 * (ak[1:] - ak[:-1]) + ak[:-1]
    era['bkm'] = 0.5 * (bk[1:] - bk[:-1]) + bk[:-1]
    return dict(c, era=era)


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_waves_that_walk_to_the_top(storage):
    """Columns with ps < ps_mono_min never vote to stop: their wave walks to level 0, through the pure-pressure levels whose
    final QV the delta kernel has written and where the e workspace holds nothing.  QV is the same on all levels."""
    dtype, ref = STORAGE[storage]
    c = _bend_one_layer(_case(23, 29, 31, seed=5, dtype=dtype), 75000.0)
    ps = c['era']['PS'].reshape(-1)
    low = np.array([(ps[i:i + 64] < 75000.0).any() for i in range(0, ps.size, 64)])
    assert low.any() and not low.all()                      # waves of both kinds
    bk = c['era']['bk']
    assert (0.5 * (bk[1:] + bk[:-1]) == 0.0).sum() > 0      # and pure-pressure levels for them to walk through
    n = _both(c, ref)[0][0]['n_iter']
    _check(_both(c, ref, dict(loop_guess=n)), TAKES_PATH[storage])


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_a_nan_surface_pressure_walks_to_the_top_too(storage):
    """NaN PS in one column: its wave never votes to stop either and stores NaN from the first hybrid level on.  The
    reference raises on the all-NaN column and so does the file, with the same message and column whatever the option
    says.  No output reaches the caller to be compared: a NaN PS leaves the column without a level at or below p_ref, which
    the loop kernel reports as "p_ref locally lies below the surface" in the file path and in functions.adjust_ps_loop alike
    (the call raises before it returns hus_pgw).  What a walk to level 0 stores is compared, with outputs, by
    test_waves_that_walk_to_the_top; this case pins that the NaN wave's stores and marks change neither the error nor the
    getter, which reports no marks used for a file that failed."""
    dtype, ref = STORAGE[storage]
    c = _case(23, 29, 31, seed=5, dtype=dtype)
    era = dict(c['era'])
    era['PS'] = c['era']['PS'].copy()
    era['PS'][0, 3, 7] = np.nan
    (a, ma), (b, mb) = _both(dict(c, era=era), ref, dict(loop_guess=6))
    assert isinstance(a, ValueError) and isinstance(b, ValueError), (a, b)
    assert str(a) == str(b) and getattr(a, 'column', None) == getattr(b, 'column', None) == 3 * 29 + 7
    assert ma == (False, 0) and mb == (False, 0)


@pytest.mark.parametrize('storage,opts', [('f64', dict(multipass=0)), ('f32ref', dict(multipass=0)),
                                          ('f64', dict(full_column=1)), ('f32ref', dict(full_column=1)),
                                          ('f64', dict(quad=0))],
                         ids=lambda v: v if isinstance(v, str) else '-'.join('%s%d' % kv for kv in v.items()))
def test_unaffected_configurations(storage, opts):
    """One launch per pass, full-column passes, and the pair kernels (quad = 0: kept as an independent cross-check, all of
    their files' QV comes from the finalize kernel; the library has them for float64 and float32 fast storage only): the
    marks are not used."""
    dtype, ref = STORAGE[storage]
    c = _case(dtype=dtype)
    _check(_both(c, ref, dict(opts, loop_guess=6)), False)


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_local_reference_level(storage):
    """settings.p_ref_inp = None: the LOCAL instantiation of the loop kernel stores nothing."""
    dtype, ref = STORAGE[storage]
    c = _case(dtype=dtype)
    n = _both(c, ref, p_ref='local')[0][0]['n_iter']
    _check(_both(c, ref, dict(loop_guess=n), p_ref='local'), False)


def _loop_both(c, guess=None, dtype=np.float64):
    """functions.adjust_ps_loop with the option on and off; returns the two results after comparing them."""
    from oracle import pgw_oracle as O
    from pgw4era5_amd import functions as F
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    era, d = c['era'], c['deltas']
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    hur = O.specific_to_relative_humidity(era['QV'], pa, era['T'])
    cast = lambda x: np.asarray(x).astype(dtype)
    old = ctx.get_option('qv_from_pass'), ctx.get_option('loop_guess')
    res = []
    try:
        for on in (1, 0):
            ctx.set_option('qv_from_pass', on)
            if guess is not None:
                ctx.set_option('loop_guess', guess)
            r = F.adjust_ps_loop(era['ak'], era['bk'], cast(era['PS']), cast(era['FIS']), cast(era['T']), cast(era['QV']),
                                 cast(era['T'] + 2.0), cast(hur - 1.0), cast(d['zg'][6, 7][None]))
            res.append((r, ctx.last_qv_from_pass()))
    finally:
        ctx.set_option('qv_from_pass', old[0])
        ctx.set_option('loop_guess', old[1])
    (a, ma), (b, mb) = res
    assert a['n_iter'] == b['n_iter']
    np.testing.assert_array_equal(np.asarray(a['max_err']), np.asarray(b['max_err']))
    np.testing.assert_array_equal(a['ps_pgw'], b['ps_pgw'])
    np.testing.assert_array_equal(a['hus_pgw'], b['hus_pgw'])
    assert mb == (False, 0) and (ma[1] > 0) == ma[0]
    return (a, ma), (b, mb)


@pytest.mark.parametrize('storage', ['f64', 'f32'])
def test_function_level_loop(storage):
    """pgw_adjust_ps_loop (qv_done_levels = 0: every level is the loop's) takes the same path: predicted exactly, the
    marks are used (float64; the float32 instantiation is the excluded one); predicted one pass short, they are not."""
    dtype = STORAGE[storage][0]
    c = _case()
    n = _loop_both(c, dtype=dtype)[0][0]['n_iter']
    assert n >= 2
    (a, ma), _ = _loop_both(c, guess=n, dtype=dtype)
    assert ma[0] == TAKES_PATH[storage]
    (a, ma), _ = _loop_both(c, guess=n - 1, dtype=dtype)    # converges in the first of two continuation passes
    assert not ma[0]
