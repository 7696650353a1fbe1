"""`pgw_delta_bracket` (the record bracketing of load_delta, functions.py:224-283, as host C on integer seconds) against
`step_03_apply_to_era.delta_time_bracket` (the same on numpy datetime64): the two indices, the dropped record and the two
abscissae - the doubles bit for bit - on monthly and daily axes, with none, one and two Feb 29 stamps, at the wrap-around of the
year, on records, one second beside them, around the end of February in leap and other years, and on a seeded sample of hourly
instants.  Host arithmetic only: the library loads without a GPU."""
import ctypes as C
import datetime as dt
import struct

import numpy as np
import pytest

S = 'datetime64[s]'


def _days(first, last, hour=12):
    return (np.arange(first, last, dtype='datetime64[D]').astype(S) + np.timedelta64(hour, 'h')).astype(S)


AXES = {
    'monthly_mid': np.array(['2000-%02d-15T12:00:00' % m for m in range(1, 13)], dtype=S),
    'daily_leap': _days('2000-01-01', '2001-01-01'),                    # 366 records, one Feb 29
    'daily_365': _days('2001-01-01', '2002-01-01'),
    'monthly_first': np.array(['1995-%02d-01T00:00:00' % m for m in range(1, 13)], dtype=S),
    # records of two leap years one after the other: the second Feb 29 is dropped, the first stays and rolls into March
    # wherever the target year has no Feb 29 (the re-yeared axis is then not sorted)
    'two_leap_days': np.concatenate([_days('2000-02-20', '2000-03-06', 6), _days('2004-02-20', '2004-03-06', 18)]),
}
assert len(AXES['daily_leap']) == 366 and len(AXES['daily_365']) == 365


def _c_bracket(lib, times, target_s):
    t = np.ascontiguousarray(times.astype(S).astype(np.int64))
    ib, ia, drop, xh, xn = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_double(-7.0), C.c_double(-7.0)
    rc = lib.pgw_delta_bracket(t.ctypes.data_as(C.POINTER(C.c_longlong)), len(t), int(target_s), C.byref(ib), C.byref(ia),
                               C.byref(xh), C.byref(xn), C.byref(drop))
    assert rc == 0
    return ib.value, ia.value, xh.value, xn.value, drop.value


def _py_bracket(s3, times, target):
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(times, target)
    gone = sorted(set(range(len(times))) - set(int(k) for k in keep))
    assert len(gone) <= 1
    return ib, ia, x_hi, x_new, (gone[0] if gone else -1)


def _bits(x):
    return struct.pack('<d', x)


def _targets(s3, times):
    """The issue's list for one axis, as datetime64[s]."""
    out = []
    for year in (2003, 2004, 2100):                                     # no Feb 29, one, none (a century year)
        out += ['%d-01-01T00:00:00' % year, '%d-01-01T00:00:01' % year, '%d-12-31T23:00:00' % year, '%d-12-31T23:59:59' % year,
                '%d-02-28T23:00:00' % year, '%d-03-01T00:00:00' % year, '%d-02-28T12:00:00' % year]
        kept = s3.delta_time_bracket(times, np.datetime64('%d-06-01' % year))[4]
        ty = np.sort(s3._reyear(times[kept], year))
        # before the first and after the last re-yeared stamp: the two wrap branches (where the axis leaves room for them)
        out += [ty[0] - np.timedelta64(1, 'h'), ty[-1] + np.timedelta64(1, 'h')]
        for r in sorted({0, 1, len(ty) // 2, len(ty) - 1}):             # on a record and one second on either side
            out += [ty[r], ty[r] - np.timedelta64(1, 's'), ty[r] + np.timedelta64(1, 's')]
    out.append('2004-02-29T12:00:00')
    return [np.datetime64(t).astype(S) for t in out]


@pytest.fixture(scope='module')
def lib():
    from pgw4era5_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('axis', sorted(AXES))
def test_listed_targets(lib, axis):
    from pgw4era5_amd import step_03_apply_to_era as s3
    times = AXES[axis]
    seen = set()
    for t in _targets(s3, times):
        want = _py_bracket(s3, times, t)
        got = _c_bracket(lib, times, t.astype(np.int64))
        assert got[:2] == want[:2] and got[4] == want[4], (axis, t, got, want)
        assert _bits(got[2]) == _bits(want[2]) and _bits(got[3]) == _bits(want[3]), (axis, t, got, want)
        seen.add('record' if want[0] == want[1] else 'between')
        if want[0] == want[1]:
            assert got[2] == 0.0 and got[3] == 0.0
    assert {'record', 'between'} <= seen


@pytest.mark.parametrize('axis', ['monthly_mid', 'daily_leap', 'daily_365', 'two_leap_days'])
def test_both_wrap_branches_are_reached(lib, axis):
    """Before the first re-yeared stamp the last record of the year before stands in, after the last one the first record of
    the year after: x_hi spans the turn of the year."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    times = AXES[axis]
    n_kept = len(times) - (1 if axis in ('daily_leap', 'two_leap_days') else 0)
    for t, hour in (('2003-01-01T00:00:00', 0), ('2003-12-31T23:00:00', 23)):
        got = _c_bracket(lib, times, np.datetime64(t).astype(S).astype(np.int64))
        assert got == _py_bracket(s3, times, np.datetime64(t))
        if axis != 'two_leap_days':
            assert (got[0], got[1]) == (n_kept - 1, 0) and 0.0 < got[3] < got[2]


def test_seeded_hourly_sample(lib):
    from pgw4era5_amd import step_03_apply_to_era as s3
    rng = np.random.default_rng(20260819)
    t0 = np.datetime64('1999-01-01T00:00:00').astype(S)
    hours = rng.integers(0, 34 * 366 * 24, 2000)
    hours = hours[t0 + hours.astype('timedelta64[h]') < np.datetime64('2033-01-01')]
    assert len(hours) > 1900
    for axis, times in AXES.items():
        for h in hours:
            t = t0 + np.timedelta64(int(h), 'h')
            want = _py_bracket(s3, times, t)
            got = _c_bracket(lib, times, t.astype(np.int64))
            assert got[:2] == want[:2] and got[4] == want[4], (axis, t, got, want)
            assert _bits(got[2]) == _bits(want[2]) and _bits(got[3]) == _bits(want[3]), (axis, t, got, want)


def test_dropped_record_is_the_last_feb_29(lib):
    times = AXES['two_leap_days']
    feb29 = [i for i, t in enumerate(times) if str(t)[5:10] == '02-29']
    assert len(feb29) == 2
    assert _c_bracket(lib, times, 0)[4] == feb29[-1]
    assert _c_bracket(lib, AXES['daily_365'], 0)[4] == -1


def test_bad_arguments_are_refused(lib):
    from pgw4era5_amd import _lib
    t = np.array([np.datetime64('2000-02-29T00:00:00').astype(S).astype(np.int64)])
    out = [C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_int()]
    refs = [C.byref(x) for x in out]
    p = t.ctypes.data_as(C.POINTER(C.c_longlong))
    assert lib.pgw_delta_bracket(p, 0, 0, *refs) == _lib.PGW_ERR_ARG           # no stamps
    assert lib.pgw_delta_bracket(p, 1, 0, *refs) == _lib.PGW_ERR_ARG           # the only stamp is the dropped Feb 29
    assert lib.pgw_delta_bracket(None, 1, 0, *refs) == _lib.PGW_ERR_ARG


def test_switch_and_its_environment_override(monkeypatch):
    from pgw4era5_amd import settings, step_03_apply_to_era as s3
    monkeypatch.delenv('PGW_FILE_PLAN', raising=False)
    assert settings.file_plan is True and s3._file_plan_on()
    monkeypatch.setattr(settings, 'file_plan', False)
    assert not s3._file_plan_on()
    monkeypatch.setenv('PGW_FILE_PLAN', '1')
    assert s3._file_plan_on()
    monkeypatch.setattr(settings, 'file_plan', True)
    monkeypatch.setenv('PGW_FILE_PLAN', '0')
    assert not s3._file_plan_on()


def test_plan_struct_matches_the_header():
    """The ctypes mirror of pgw_file_plan: constants and member order as include/pgw_hip.h states them."""
    import os
    import re
    from pgw4era5_amd import _lib
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pgw_hip.h')).read()
    assert int(re.search(r'#define PGW_PLAN_MAX_AXES (\d+)', txt).group(1)) == _lib.PLAN_MAX_AXES
    body = re.search(r'enum pgw_plan_var_id \{(.*?)PGW_PV_COUNT', re.sub(r'/\*.*?\*/', '', txt, flags=re.S), flags=re.S).group(1)
    names = [n.lower()[len('pgw_pv_'):] for n in re.findall(r'PGW_PV_[A-Z_]+', body)]
    assert tuple(names) == _lib.PLAN_VARS
    assert _lib.FilePlan.args.offset == 0 and _lib.FilePlan.n_axes.offset == C.sizeof(_lib.FileArgs)
    assert C.sizeof(_lib.PlanVar) == 32 and C.sizeof(_lib.FilePlan) == C.sizeof(_lib.FileArgs) + 8 + 8 * 8 + 4 * 8 + 32 * 11


def test_instant_to_whole_seconds():
    """What process_file_device hands to the library: seconds since 1970-01-01, or None (-> the host-built struct) for an
    instant with a sub-second part or a time zone."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    d = dt.datetime(2006, 3, 15, 12, 30, 7)
    want = int(np.datetime64(d).astype(S).astype(np.int64))
    assert s3._whole_seconds(d) == want
    assert s3._whole_seconds(np.datetime64(d)) == want
    assert s3._whole_seconds('2006-03-15T12:30:07') == want
    assert s3._whole_seconds(dt.datetime(1969, 12, 31, 23, 59, 59)) == -1
    assert s3._whole_seconds(d.replace(microsecond=5)) is None
    assert s3._whole_seconds(d.replace(tzinfo=dt.timezone.utc)) is None
    assert s3._whole_seconds(np.datetime64('2006-03-15T12:30:07.250')) is None
