"""CPU-side checks of the step_01 climatologies and climate deltas: calendars, bins, command line, C-ABI bookkeeping.
No compute call is made here; the kernels and the file functions are checked in tests/test_step01_clim_hip.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ymd(values, units, calendar):
    from pgw4era5_amd import ncio
    y, m, d = ncio.cf_year_month_day(values, units, calendar)
    for a in (y, m, d):
        assert a.dtype.kind == 'i' and a.shape == np.shape(values)
    return [tuple(int(v) for v in row) for row in zip(y, m, d)]


def test_new_entries_are_declared_bound_and_have_kernel_ids():
    from pgw4era5_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    for name in ('pgw_clim_accumulate', 'pgw_field_sub', 'pgw_test_read_records'):
        assert name in _lib.SIGNATURES and name + '(' in hdr
    for kid, cname in (('clim_accumulate', 'PGW_K_CLIM_ACCUMULATE'), ('field_sub', 'PGW_K_FIELD_SUB'), ('clim_read', 'PGW_K_CLIM_READ')):
        assert '%s = %d' % (cname, _lib.KERNEL_IDS[kid]) in hdr
    assert 'PGW_K_COUNT = %d' % len(_lib.KERNEL_IDS) in hdr
    assert sorted(_lib.KERNEL_IDS.values()) == list(range(len(_lib.KERNEL_IDS)))
    # the header entries cite the script lines they replace
    assert 'extract_climate_delta.sh:153-159, 217-219' in hdr and 'extract_climate_delta.sh:244-249' in hdr
    res, args = _lib.SIGNATURES['pgw_clim_accumulate']
    assert len(args) == 11
    assert len(_lib.SIGNATURES['pgw_field_sub'][1]) == 6


@pytest.mark.parametrize('cal', ['standard', 'gregorian', 'proleptic_gregorian'])
def test_ymd_gregorian(cal):
    u = 'days since 1850-01-01 00:00:00'
    d0 = int((np.datetime64('2003-12-31') - np.datetime64('1850-01-01')).astype(np.int64))
    assert _ymd([d0, d0 + 0.999, d0 + 1], u, cal) == [(2003, 12, 31), (2003, 12, 31), (2004, 1, 1)]
    f28 = int((np.datetime64('2004-02-28') - np.datetime64('1850-01-01')).astype(np.int64))
    assert _ymd([f28, f28 + 1.5, f28 + 2], u, cal) == [(2004, 2, 28), (2004, 2, 29), (2004, 3, 1)]
    f28 = int((np.datetime64('2100-02-28') - np.datetime64('1850-01-01')).astype(np.int64))          # no leap year
    assert _ymd([f28 + 0.25, f28 + 1], u, cal) == [(2100, 2, 28), (2100, 3, 1)]
    # other units, a reference instant that is not midnight
    assert _ymd([0, 11, 12, 36], 'hours since 2000-02-28 12:00:00', cal) == [(2000, 2, 28), (2000, 2, 28), (2000, 2, 29), (2000, 3, 1)]
    assert _ymd([86399, 86400], 'seconds since 1999-12-31', cal) == [(1999, 12, 31), (2000, 1, 1)]


@pytest.mark.parametrize('cal', ['noleap', '365_day'])
def test_ymd_noleap_and_decode_cf_time_agree(cal):
    from pgw4era5_amd import ncio
    u = 'days since 1850-1-1 00:00:00'
    y0 = (2004 - 1850) * 365
    assert _ymd([y0 - 0.5, y0, y0 + 58.75, y0 + 59, y0 + 364.99, y0 + 365], u, cal) == \
        [(2003, 12, 31), (2004, 1, 1), (2004, 2, 28), (2004, 3, 1), (2004, 12, 31), (2005, 1, 1)]
    # month and day of decode_cf_time (which maps noleap dates onto the standard calendar) agree by construction
    rng = np.random.default_rng(0)
    vals = np.sort(rng.uniform(0, 400 * 365, 500))
    vals = np.concatenate([vals, np.arange(y0 - 3, y0 + 370) + 0.5])
    y, m, d = ncio.cf_year_month_day(vals, u, cal)
    t = ncio.decode_cf_time(vals, u, cal)
    assert np.array_equal(y, t.astype('datetime64[Y]').astype(np.int64) + 1970)
    assert np.array_equal(m, (t.astype('datetime64[M]') - t.astype('datetime64[Y]').astype('datetime64[M]')).astype(np.int64) + 1)
    assert np.array_equal(d, (t.astype('datetime64[D]') - t.astype('datetime64[M]').astype('datetime64[D]')).astype(np.int64) + 1)
    assert not ((m == 2) & (d == 29)).any()


@pytest.mark.parametrize('cal', ['all_leap', '366_day'])
def test_ymd_all_leap(cal):
    u = 'days since 2001-01-01'
    assert _ymd([0, 58, 59.5, 60, 365, 366, 366 + 59], u, cal) == \
        [(2001, 1, 1), (2001, 2, 28), (2001, 2, 29), (2001, 3, 1), (2001, 12, 31), (2002, 1, 1), (2002, 2, 29)]


def test_ymd_360_day_is_not_clipped():
    u = 'days since 2000-01-01'
    assert _ymd([0, 29, 30, 57, 58, 59.9, 60, 359, 360, 360 + 58.5], u, '360_day') == \
        [(2000, 1, 1), (2000, 1, 30), (2000, 2, 1), (2000, 2, 28), (2000, 2, 29), (2000, 2, 30), (2000, 3, 1), (2000, 12, 30),
         (2001, 1, 1), (2001, 2, 29)]
    # values before the reference instant
    assert _ymd([-1, -0.25], u, '360_day') == [(1999, 12, 30), (1999, 12, 30)]


def test_ymd_errors():
    from pgw4era5_amd import ncio
    with pytest.raises(ValueError):
        ncio.cf_year_month_day([0], 'days since 2000-01-01', 'julian')
    with pytest.raises(ValueError):
        ncio.cf_year_month_day([0], 'fortnights since 2000-01-01', 'noleap')
    with pytest.raises(ValueError):
        ncio.cf_year_month_day([0], 'days after 2000', 'noleap')


def test_calendar_bins_keys_order_and_years():
    from pgw4era5_amd import step_01_extract_deltas as s1
    u = 'days since 2000-01-01'
    # a file that is NOT in calendar order within the year: it starts in November
    t = np.arange(304, 304 + 2 * 365) + 0.5
    keys, bins = s1.calendar_bins(t, u, 'noleap', 'ymonmean')
    assert keys.tolist() == list(range(1, 13)) and bins.shape == t.shape and bins.dtype.kind == 'i'
    assert bins[0] == 10 and bins[29] == 10 and bins[30] == 11 and bins[61] == 0           # Nov, Nov 30, Dec 1, Jan 1
    assert np.bincount(bins).tolist() == [62, 56, 62, 60, 62, 60, 62, 62, 60, 62, 60, 62]
    keys, bins = s1.calendar_bins(t, u, 'noleap', 'ydaymean')
    assert len(keys) == 365 and keys[0] == 101 and keys[-1] == 1231 and np.all(np.diff(keys) > 0) and 229 not in keys
    assert keys[bins[0]] == 1101 and np.all(np.bincount(bins) == 2)
    # a Gregorian axis over a leap year: Feb 29 is a bin of its own
    t = np.arange(0, 366 + 365) + 0.5
    keys, bins = s1.calendar_bins(t, u, 'proleptic_gregorian', 'ydaymean')
    assert len(keys) == 366 and keys[59] == 229
    cnt = np.bincount(bins)
    assert cnt[59] == 1 and np.all(np.delete(cnt, 59) == 2)
    # selyear: everything else is bin -1; keys are those of the kept records only
    keys, bins = s1.calendar_bins(t, u, 'proleptic_gregorian', 'ydaymean', years=(2001, 2001))
    assert len(keys) == 365 and 229 not in keys and np.all(bins[:366] == -1) and bins[366:].tolist() == list(range(365))
    keys, bins = s1.calendar_bins(t, u, 'proleptic_gregorian', 'ymonmean', years=(2000, 2000))
    assert keys.tolist() == list(range(1, 13)) and np.all(bins[366:] == -1) and np.bincount(bins[:366])[1] == 29
    keys, bins = s1.calendar_bins(t, u, 'proleptic_gregorian', 'ymonmean', years=(1990, 1999))
    assert len(keys) == 0 and np.all(bins == -1)
    # 360_day keeps Feb 30 as a key
    keys, _ = s1.calendar_bins(np.arange(360) + 0.5, u, '360_day', 'ydaymean')
    assert len(keys) == 360 and 230 in keys and 131 not in keys
    with pytest.raises(ValueError):
        s1.calendar_bins(t, u, 'noleap', 'yseasmean')


def test_argument_surface_of_the_new_sub_commands():
    from pgw4era5_amd import step_01_extract_deltas as s1
    p = s1.build_parser()
    a = p.parse_args(['climatology', '-i', 'a_{}.nc', 'b_{}.nc', '-o', 'out_{}.nc', '-v', 'ta,hur', '-m', 'ydaymean'])
    assert (a.command, a.input, a.output, a.var_names, a.mode) == ('climatology', ['a_{}.nc', 'b_{}.nc'], 'out_{}.nc', 'ta,hur', 'ydaymean')
    assert a.years is None and a.max_records is None and a.out_dtype is None
    a = p.parse_args(['climatology', '-i', 'a.nc', '-o', 'b.nc', '-v', 'ta', '-m', 'ymonmean', '-y', '1985/2014', '--max_records', '5',
                      '--out_dtype', 'float64'])
    assert a.input == ['a.nc'] and a.years == '1985/2014' and a.max_records == 5 and a.out_dtype == 'float64'
    assert s1._parse_years(a.years) == (1985, 2014) and s1._parse_years(None) is None
    d = p.parse_args(['delta', 'scen.nc', 'hist.nc', 'delta.nc', '-v', 'ta'])
    assert (d.command, d.scen_file, d.hist_file, d.delta_file, d.var_names) == ('delta', 'scen.nc', 'hist.nc', 'delta.nc', 'ta')
    for bad in (['climatology', '-i', 'a', '-o', 'b', '-v', 'ta'], ['climatology', '-i', 'a', '-o', 'b', '-v', 'ta', '-m', 'yearmean'],
                ['delta', 'a', 'b', '-v', 'ta'], ['delta', 'a', 'b', 'c']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(ValueError):                                # several variables, no {} in the paths
        s1.main(['climatology', '-i', 'a_{}.nc', 'b.nc', '-o', 'c_{}.nc', '-v', 'ta,ua', '-m', 'ymonmean'])
    with pytest.raises(ValueError):
        s1.main(['delta', 's_{}.nc', 'h_{}.nc', 'd.nc', '-v', 'ta,ua'])
    with pytest.raises(ValueError):
        s1._parse_years('1985')
    # the earlier sub-commands parse as before
    h = p.parse_args(['hus_to_hur', 'hus.nc', 'ta.nc', 'hur.nc', '-a', 'amon.nc'])
    assert h.command == 'hus_to_hur'


def test_help_of_the_new_sub_commands_runs_without_the_library():
    env = dict(os.environ, PGW_LIB=os.path.join(ROOT, 'no_such_dir', 'libpgw_hip.so'), PYTHONPATH=ROOT)
    for argv in (['climatology', '--help'], ['delta', '--help']):
        r = subprocess.run([sys.executable, '-m', 'pgw4era5_amd.step_01_extract_deltas'] + argv, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert 'usage' in r.stdout


def test_argument_checks_before_any_launch():
    from pgw4era5_amd import step_01_extract_deltas as s1
    x = np.zeros((4, 2, 3), np.float64)
    with pytest.raises(ValueError):
        s1.climatology(x, [0, 0, 1], 2)                            # one bin entry per record
    with pytest.raises(ValueError):
        s1.climatology(x, [0, 0, 1, 1], 0)
    with pytest.raises(ValueError):
        s1.climatology(x, [0, 0, 1, 1], 2, out_dtype='float32')    # float64 records cannot be narrowed
    with pytest.raises(ValueError):
        s1.climatology(x, [0, 0, 1, 5], 2)
    with pytest.raises(ValueError):
        s1.climatology_files([], 'out.nc', 'ta', 'ymonmean')
    with pytest.raises(ValueError):
        s1.climatology_files(['a.nc'], 'out.nc', 'ta', 'daymean')


def test_fill_encoding_of_the_output():
    from pgw4era5_amd import step_01_extract_deltas as s1
    v = np.array([1.0, np.nan, 3.0], np.float32)
    out, attrs = s1._encoded(v.copy(), dict(units='K', _FillValue=np.float64(1e20), missing_value=np.float32(1e20), scale_factor=2.0))
    assert out.dtype == np.float32 and out[1] == np.float32(1e20) and out[0] == 1 and set(attrs) == {'units', '_FillValue', 'missing_value'}
    assert attrs['_FillValue'].dtype == np.float32 and attrs['missing_value'].dtype == np.float32
    out, attrs = s1._encoded(v.copy(), dict(units='K'))               # no fill value: NaN stays
    assert np.isnan(out[1]) and attrs == dict(units='K')
    out, attrs = s1._encoded(v.astype(np.float64), dict(missing_value=np.float32(-999.0)))
    assert out.dtype == np.float64 and out[1] == -999.0 and attrs['missing_value'].dtype == np.float64
