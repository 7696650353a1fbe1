"""
step_01: the array programs of the reference's step_01_extract_deltas directory on MI355X.

* `CFday_interp_to_plev.py:86-154`: daily CMIP6 `CFday` fields on the GCM's hybrid model levels (`ap`, `b`, `ps` in the
  file) interpolated to a fixed list of pressure levels -> `interp_to_plev` / `interp_file` / sub-command `interp_to_plev`.
  One fused kernel (`pgw_interp_hybrid_to_plev`): the source pressure `ap + b * ps` is formed per column in registers and
  the logarithms of the target list are taken once per thread block; neither 4-D pressure field of the reference
  (`source_P`, `targ_P`, :91 and :115-122) exists on the host or on the device.
* `Emon_convert_hus_to_hur.py:16-21, 45-123`: monthly `Emon` specific humidity -> relative humidity with the script's own
  Magnus formula (`specific_to_relative_humidity` HERE is that one; `functions.specific_to_relative_humidity` is the IFS
  formula of the reference's functions.py), then the coarse `Amon` hur carried onto the finer `Emon` levels with weights
  taken from the computed hur (`merge_hur_levels`) -> `hus_to_hur_file` / sub-command `hus_to_hur`.

* `extract_climate_delta.sh:153-159, 217-219, 235-238, 244-249`: the array program inside the shell template - `cdo -cat`,
  `-selyear`, `ymonmean` / `ydaymean` of the historical and of the scenario series and `cdo sub` of the two ->
  `calendar_bins` / `climatology` / `climatology_files` / `delta_files`, sub-commands `climatology` and `delta`.  The mean
  of a bin is the sequential float64 sum of its records in time order, missing values skipped, divided by their count
  (`pgw_clim_accumulate`); the difference is `pgw_field_sub`.  `cdo` itself is not available to this project and the
  reference has no program text for this step: the definition of correct is that statement plus cdo's documented
  conventions (date of the last contributing record, records sorted by month / day key); bit parity with cdo is unpinned
  (kind U).

The rest of the shell templates of step_01 (site paths, `sellonlatbox`, the Emon model-top merge, `wget`) are site scripts
and stay out of scope.

Array kinds as in `functions.py`: numpy, `ncio.Field` (labels re-wrapped) or `DeviceArray` in, the same kind out.
Files are NetCDF-3 through `ncio` like everywhere in this package.
"""
import argparse
import os

import numpy as np

from . import _lib, ncio
from .device import DeviceArray, default_context, dtype_tag
from ._lib import _dp, _ip
from .operands import F32, F64, check_extrapolate, dev, is_labelled, out_like, raw
from .settings import LAT_GCM, LEV_GCM, LON_GCM, PLEV_GCM, TIME_GCM

MAX_LEVELS = 256          # nsrc, ntarg, nplev limit of the kernels (include/pgw_hip.h)


def _f64(x, name):
    a = np.ascontiguousarray(raw(x), dtype=np.float64)
    if a.ndim != 1:
        raise ValueError('%s must be one-dimensional' % name)
    return a


def _cdp(a):
    return a.ctypes.data_as(_dp)


# ------------------------------------------------------------------------------- model levels -> pressure levels
def levels_descend(ap, b, ps_ref=1.0e5):
    """True when pressure ap + b * ps FALLS with the level index (the file stores the surface first), which is the order
    the reference assumes when it reverses `lev` (CFday_interp_to_plev.py:89)."""
    ap, b = _f64(ap, 'ap'), _f64(b, 'b')
    return bool(ap[0] + b[0] * ps_ref > ap[-1] + b[-1] * ps_ref)


def _launch_hybrid(ctx, d_var, d_ps, ap, b, targ, mode, src_rev, out_rev, d_out):
    nt, S = d_var.shape[0], d_var.shape[1]
    ncol = int(np.prod(d_var.shape[2:], dtype=np.int64))
    ctx._check(ctx.lib.pgw_interp_hybrid_to_plev(ctx.handle, dtype_tag(d_var.dtype), dtype_tag(d_out.dtype), nt, S, len(targ), ncol,
                                                 d_var.ptr, d_ps.ptr, _cdp(ap), _cdp(b), _cdp(targ), mode,
                                                 1 if src_rev else 0, 1 if out_rev else 0, d_out.ptr))


def _hybrid_args(var_dtype, ps_dtype, S, ap, b, targ_plev, out_dtype):
    ap, b = _f64(ap, 'ap'), _f64(b, 'b')
    if len(ap) != S or len(b) != S:
        raise ValueError('Level dimension of var and ap / b is inconsistent!')
    if not 2 <= S <= MAX_LEVELS:
        raise ValueError('between 2 and %d model levels are supported, got %d' % (MAX_LEVELS, S))
    targ = np.sort(_f64(targ_plev, 'targ_plev'))                   # CFday_interp_to_plev.py:114
    if not 1 <= len(targ) <= MAX_LEVELS:
        raise ValueError('between 1 and %d target levels are supported, got %d' % (MAX_LEVELS, len(targ)))
    # float32 var with float32 ps is the CFday file's dtype flow; anything mixed is computed in float64
    dt = F32 if (np.dtype(var_dtype) == F32 and np.dtype(ps_dtype) == F32) else F64
    odt = F64 if out_dtype is None else np.dtype(out_dtype)
    if odt not in (F32, F64) or (odt == F32 and dt != F32):
        raise ValueError('out_dtype: float64, or float32 for float32 input')
    return ap, b, targ, dt, odt


def interp_to_plev(var, ps, ap, b, targ_plev, extrapolate='constant', lev_descending=None, out_dtype=None,
                   plev_descending=True):
    """CFday_interp_to_plev.py:89-134 on arrays: `var` (time, lev, lat, lon) on hybrid levels of pressure
    ap[lev] + b[lev] * ps, `ps` (time, lat, lon) -> (time, plev, lat, lon) on the pressure levels `targ_plev`, linear in
    ln p (functions.interp_logp_4d with the same `extrapolate` modes and errors).

    targ_plev is sorted ascending (:114); the result comes with pressure DESCENDING along its level axis (:133-134)
    unless plev_descending=False.  lev_descending: the level axis of var / ap / b runs from the surface upwards and is
    read in reverse (:89); None decides from ap and b (`levels_descend`).
    Dtypes: float32 var and ps give the reference's result on float32 files - a float64 array in which only
    `src_y[i2] - src_y[i1]` was taken in float32 (numba, functions.py:575-578); float64 input is plain float64.
    out_dtype='float32' (float32 input only) narrows that float64 result on the store: half the output, not the
    reference's bits.
    Labelled input comes back as `ncio.Field` on (time, plev, lat, lon) with the `plev` coordinate."""
    mode = check_extrapolate(extrapolate)
    rv, rp = raw(var), raw(ps)
    if len(rv.shape) != 4:
        raise ValueError('expected a 4-D (time, lev, lat, lon) array, got shape %s' % (rv.shape,))
    nt, S, nlat, nlon = rv.shape
    if tuple(rp.shape) != (nt, nlat, nlon):
        raise ValueError('ps must be (time, lat, lon) = %s, got %s' % ((nt, nlat, nlon), tuple(rp.shape)))
    ap, b, targ, dt, odt = _hybrid_args(rv.dtype, rp.dtype, S, ap, b, targ_plev, out_dtype)
    src_rev = levels_descend(ap, b) if lev_descending is None else bool(lev_descending)
    ctx = default_context()
    d_var, d_ps = dev(ctx, var, dt), dev(ctx, ps, dt)
    out = ctx.empty((nt, len(targ), nlat, nlon), odt)
    _launch_hybrid(ctx, d_var, d_ps, ap, b, targ, mode, src_rev, plev_descending, out)
    if isinstance(rv, DeviceArray):
        return out
    host = out.numpy()
    if is_labelled(var):
        dims = tuple(var.dims)
        coords = {d: var.coords[d] for d in (dims[0], dims[2], dims[3]) if d in getattr(var, 'coords', {})}
        coords[PLEV_GCM] = targ[::-1].copy() if plev_descending else targ
        return ncio.Field(host, (dims[0], PLEV_GCM, dims[2], dims[3]), coords, dict(getattr(var, 'attrs', {})),
                          getattr(var, 'name', None))
    return host


def load_target_plev(path):
    """The target list: a text file of numbers (np.loadtxt, CFday_interp_to_plev.py:114), returned ascending."""
    return np.sort(np.atleast_1d(np.loadtxt(path)).astype(np.float64).reshape(-1))


def records_per_block(ctx, nrec, S, N, ncol, s_in, s_out, max_records=None):
    """Time records per launch: what fits into 80 % of the card's free memory (`pgw_mem_info`), at most `max_records`."""
    return _fit_records(ctx, nrec, (S * s_in + s_in + N * s_out) * ncol, max_records)


def _fit_records(ctx, nrec, bytes_per_record, max_records=None):
    free, _ = ctx.mem_info()
    n = max(1, min(int(nrec), int(0.8 * free) // max(bytes_per_record, 1)))
    if max_records:
        n = max(1, min(n, int(max_records)))
    return n


def interp_file(inp_path, out_path, var_name, targ_plev, extrapolate='constant', max_records=None, out_dtype=None):
    """CFday_interp_to_plev.py:86-154 for one file: `var_name` (time, lev, lat, lon) with `ap`, `b` (lev) and `ps`
    (time, lat, lon) of `inp_path` -> `var_name` (time, plev, lat, lon) with pressure descending, coordinates time /
    plev / lat / lon, the attributes of time, lon, lat and the variable carried over (:138-151).  As in the reference the
    level axis is taken to run from the surface upwards and is reversed (:89).

    The file goes through in blocks of time records (`ncio.RecordReader`), so it may be larger than the card's memory;
    `max_records` caps the block (the results do not depend on it)."""
    mode = check_extrapolate(extrapolate)
    targ = load_target_plev(targ_plev) if isinstance(targ_plev, (str, os.PathLike)) else np.sort(_f64(targ_plev, 'targ_plev'))
    ds = ncio.open_dataset(inp_path, decode_times=False, skip=(var_name, 'ps'))
    for need in (var_name, 'ps', 'ap', 'b'):
        if need not in ds:
            raise KeyError(need)
    vdims = tuple(ds[var_name].dims)
    if vdims != (TIME_GCM, LEV_GCM, LAT_GCM, LON_GCM):
        raise ValueError('%s must be on (%s, %s, %s, %s), got %s' % (var_name, TIME_GCM, LEV_GCM, LAT_GCM, LON_GCM, vdims))
    if tuple(ds['ps'].dims) != (TIME_GCM, LAT_GCM, LON_GCM):
        raise ValueError('ps must be on (%s, %s, %s), got %s' % (TIME_GCM, LAT_GCM, LON_GCM, tuple(ds['ps'].dims)))
    rv, rp = ncio.RecordReader(inp_path, var_name, decode_times=False), ncio.RecordReader(inp_path, 'ps', decode_times=False)
    try:
        nrec, (S, nlat, nlon) = rv.nrec, rv.rec_shape
        ap, b, targ, dt, odt = _hybrid_args(rv.dtype, rp.dtype, S, ds['ap'].values, ds['b'].values, targ, out_dtype)
        N, ncol = len(targ), nlat * nlon
        ctx = default_context()
        nb = records_per_block(ctx, nrec, S, N, ncol, dt.itemsize, odt.itemsize, max_records)
        result = np.empty((nrec, N, nlat, nlon), dtype=odt)
        d_var, d_ps, d_out = ctx.empty((nb, S, nlat, nlon), dt), ctx.empty((nb, nlat, nlon), dt), ctx.empty((nb, N, nlat, nlon), odt)
        h_var, h_ps = np.empty((nb, S, nlat, nlon), dtype=dt), np.empty((nb, nlat, nlon), dtype=dt)
        for r0 in range(0, nrec, nb):
            n = min(nb, nrec - r0)
            for i in range(n):
                h_var[i], h_ps[i] = rv.read_record(r0 + i), rp.read_record(r0 + i)
            v, p, o = d_var, d_ps, d_out
            if n != nb:                                           # last, shorter block: leading records of the same buffers
                v = DeviceArray(ctx, (n, S, nlat, nlon), dt, ptr=d_var.ptr, owner=d_var)
                p = DeviceArray(ctx, (n, nlat, nlon), dt, ptr=d_ps.ptr, owner=d_ps)
                o = DeviceArray(ctx, (n, N, nlat, nlon), odt, ptr=d_out.ptr, owner=d_out)
            v.copy_from(h_var[:n]); p.copy_from(h_ps[:n])
            _launch_hybrid(ctx, v, p, ap, b, targ, mode, True, True, o)
            result[r0:r0 + n] = o.numpy()
    finally:
        rv.close(); rp.close()
    src = ds[var_name]
    coords = {d: ds[d].values for d in (TIME_GCM, LAT_GCM, LON_GCM) if d in ds}
    coords[PLEV_GCM] = targ[::-1].copy()
    out = ncio.Dataset(record_dim=ds.record_dim)
    for d in (TIME_GCM, PLEV_GCM, LAT_GCM, LON_GCM):
        if d in coords:
            out[d] = ncio.Field(coords[d], (d,), {d: coords[d]}, dict(ds[d].attrs) if d in ds else {})
    out[var_name] = ncio.Field(result, (TIME_GCM, PLEV_GCM, LAT_GCM, LON_GCM), coords, dict(src.attrs))
    ncio.to_netcdf(out, out_path)
    return out_path


# ------------------------------------------------------------------------------- Emon hus -> hur
def specific_to_relative_humidity(QV, P, T):
    """Emon_convert_hus_to_hur.py:16-21: RH = 0.263 * P * QV * (exp(17.67 * (T - 273.15) / (T - 29.65)))**(-1).
    QV, T (time, plev, lat, lon) of one dtype; P: the 1-D `plev` coordinate in Pa (the script broadcasts it to a 4-D array
    first, :53-55; a 4-D P whose columns all hold that list is accepted and reduced to it).  The result is float64 as
    numpy gives it with a float64 P: on float32 QV / T the exponent, exp and the reciprocal are float32 operations, the
    products float64."""
    rq, rt = raw(QV), raw(T)
    if tuple(rq.shape) != tuple(rt.shape) or len(rq.shape) != 4:
        raise ValueError('QV and T must be 4-D (time, plev, lat, lon) arrays of one shape')
    nt, nplev, nlat, nlon = rq.shape
    p = np.asarray(raw(P), dtype=np.float64) if not isinstance(raw(P), DeviceArray) else raw(P).numpy().astype(np.float64)
    if p.ndim == 4:
        if p.shape != tuple(rq.shape) or not np.array_equal(p, np.broadcast_to(p[0, :, 0, 0][None, :, None, None], p.shape), equal_nan=True):
            raise ValueError('a 4-D P must hold the same pressure list in every column')
        p = p[0, :, 0, 0]
    p = np.ascontiguousarray(p.reshape(-1))
    if len(p) != nplev or nplev > MAX_LEVELS:
        raise ValueError('P must hold the %d pressure levels of QV (at most %d)' % (nplev, MAX_LEVELS))
    dt = F32 if (rq.dtype == F32 and rt.dtype == F32) else F64
    ctx = default_context()
    d_q, d_t = dev(ctx, QV, dt), dev(ctx, T, dt)
    out = ctx.empty(rq.shape, F64)
    ctx._check(ctx.lib.pgw_magnus_rh(ctx.handle, dtype_tag(dt), nt, nplev, nlat * nlon, d_q.ptr, _cdp(p), d_t.ptr, out.ptr))
    return out_like(out, QV)


def merge_level_table(plev, amon_plev):
    """Level bookkeeping of Emon_convert_hus_to_hur.py:82-122 for the Emon levels `plev` and the Amon levels `amon_plev`:
    int32 arrays (copy_from, e_above, e_below, a_above, a_below) of len(plev), -1 where unused.
    copy_from[l] >= 0: the level is an Amon level and takes Amon's values (:120-122).  Otherwise a_below / a_above are the
    nearest Amon levels of higher / lower pressure (:85-89) and e_below / e_above the Emon indices of those pressures (:95-96).
    ValueError: no Amon level on one side (xarray's argmin / argmax of an all-NaN slice); KeyError: the neighbouring Amon
    level is not an Emon level (`hur.sel`)."""
    plev, amon = _f64(plev, 'plev'), _f64(amon_plev, 'amon_plev')
    n = len(plev)
    tabs = [np.full(n, -1, dtype=np.int32) for _ in range(5)]
    copy_from, e_above, e_below, a_above, a_below = tabs
    for l, p in enumerate(plev):
        hit = np.nonzero(amon == p)[0]
        if len(hit):
            copy_from[l] = hit[0]
            continue
        d = amon - p
        below, above = np.where(d > 0, amon, np.nan), np.where(d < 0, amon, np.nan)
        if np.all(np.isnan(below)) or np.all(np.isnan(above)):
            raise ValueError('All-NaN slice encountered: plev %r lies outside the Amon levels' % (p,))
        ib, ia = int(np.nanargmin(below)), int(np.nanargmax(above))
        for i, dst in ((ia, e_above), (ib, e_below)):             # hur.sel(plev=plev_above), then plev_below (:95-96)
            e = np.nonzero(plev == amon[i])[0]
            if not len(e):
                raise KeyError(float(amon[i]))
            dst[l] = e[0]
        a_above[l], a_below[l] = ia, ib
    return tuple(tabs)


def _same_coords(a, b, what):
    for d in (TIME_GCM, LAT_GCM, LON_GCM):
        ca, cb = getattr(a, 'coords', {}).get(d), getattr(b, 'coords', {}).get(d)
        if ca is None or cb is None:
            continue
        if np.shape(ca) != np.shape(cb) or not np.array_equal(np.asarray(ca), np.asarray(cb)):
            raise ValueError('%s: the %s coordinates differ; the fields must be on equal time / lat / lon coordinates '
                             '(nothing is aligned here)' % (what, d))


def merge_hur_levels(hur, plev, amon_hur, amon_plev):
    """Emon_convert_hus_to_hur.py:82-122: the coarse `amon_hur` (time, amon_plev, lat, lon) on the finer levels `plev` of the
    computed `hur` (time, plev, lat, lon).  Levels present in Amon take its values; every other level takes
    amon_above * w_above + amon_below * w_below with w_above = 1 - a / (a + b), w_below = 1 - b / (a + b),
    a = |hur_l - hur_above|, b = |hur_l - hur_below| (0 / 0 = NaN kept, as in the reference).  Result float64.
    xarray would align the two fields on their coordinates; here labelled inputs must have EQUAL time / lat / lon
    coordinates (ValueError otherwise).  plev / amon_plev = None: taken from the fields' `plev` coordinates."""
    if plev is None:
        plev = hur.coords[PLEV_GCM]
    if amon_plev is None:
        amon_plev = amon_hur.coords[PLEV_GCM]
    if is_labelled(hur) and is_labelled(amon_hur):
        _same_coords(hur, amon_hur, 'merge_hur_levels')
    rh, ra = raw(hur), raw(amon_hur)
    if len(rh.shape) != 4 or len(ra.shape) != 4:
        raise ValueError('hur and amon_hur must be 4-D (time, plev, lat, lon)')
    nt, nplev, nlat, nlon = rh.shape
    if (ra.shape[0], ra.shape[2], ra.shape[3]) != (nt, nlat, nlon):
        raise ValueError('hur %s and amon_hur %s differ in time / lat / lon' % (tuple(rh.shape), tuple(ra.shape)))
    tabs = merge_level_table(plev, amon_plev)
    if len(tabs[0]) != nplev or len(_f64(amon_plev, 'amon_plev')) != ra.shape[1] or nplev > MAX_LEVELS:
        raise ValueError('plev / amon_plev do not match the level axes of the fields')
    adt = F32 if ra.dtype == F32 else F64
    ctx = default_context()
    d_h, d_a = dev(ctx, hur, F64), dev(ctx, amon_hur, adt)
    out = ctx.empty(rh.shape, F64)
    ti = [np.ascontiguousarray(t, dtype=np.int32) for t in tabs]
    ctx._check(ctx.lib.pgw_hur_merge_levels(ctx.handle, dtype_tag(adt), nt, nplev, ra.shape[1], nlat * nlon, d_h.ptr, d_a.ptr,
                                            *[t.ctypes.data_as(_ip) for t in ti], out.ptr))
    return out_like(out, hur)


def hus_to_hur_file(hus_file, ta_file, hur_file, amon_hur_file):
    """Emon_convert_hus_to_hur.py:45-164 without its matplotlib figure (:126-140): files opened raw (decode_cf=False)."""
    ta = ncio.open_dataset(ta_file, decode_times=False)['ta']
    ds = ncio.open_dataset(hus_file, decode_times=False)
    hus = ds['hus']
    if hus.shape != ta.shape:                                     # :57-60
        print(hus.shape)
        print(ta.shape)
        raise ValueError()
    if tuple(hus.dims) != (TIME_GCM, PLEV_GCM, LAT_GCM, LON_GCM):
        raise ValueError('hus must be on (%s, %s, %s, %s), got %s' % (TIME_GCM, PLEV_GCM, LAT_GCM, LON_GCM, tuple(hus.dims)))
    _same_coords(hus, ta, 'hus / ta')
    hur = specific_to_relative_humidity(hus, ds[PLEV_GCM].values, ta)          # :53-62
    amon_hur = ncio.open_dataset(amon_hur_file, decode_times=False)['hur']      # :76
    hur_interp = merge_hur_levels(hur, None, amon_hur, None)                   # :78-122
    out = ncio.Dataset({k: v for k, v in ds.variables.items() if k != 'hus'}, dict(ds.attrs), ds.record_dim)     # :143-145
    attrs = {}
    for key, val in hus.attrs.items():                            # :155-161, as written: only long_name ends up renamed
        if key == 'standard_name':
            attrs[key] = 'relative_humidity'
        if key == 'long_name':
            attrs[key] = 'Relative Humidity'
        else:
            attrs[key] = val
    out['hur'] = ncio.Field(hur_interp.values, hus.dims, hus.coords, attrs)
    out.attrs['variable_id'] = 'hur'                              # :146
    ncio.to_netcdf(out, hur_file)
    return hur_file


# ------------------------------------------------------------------------------- climatologies and climate deltas
CLIM_MODES = ('ymonmean', 'ydaymean')


def calendar_bins(time_values, units, calendar, mode, years=None):
    """The bins of `cdo ymonmean` (key = month) / `cdo ydaymean` (key = month * 100 + day; Feb 29 is a bin of its own with
    fewer samples, which is why functions.load_delta drops a leap day) for the raw time coordinate of a file, in the
    file's own calendar (`ncio.cf_year_month_day`).  years=(y0, y1): only records with y0 <= year <= y1 (`cdo selyear`).
    Returns (keys, bin_of_record): the keys that occur, ascending, and per record the index of its key, -1 for records
    outside `years`."""
    if mode not in CLIM_MODES:
        raise ValueError('mode must be one of %s, got %r' % (CLIM_MODES, mode))
    year, month, day = ncio.cf_year_month_day(np.asarray(time_values).reshape(-1), units, calendar)
    key = month if mode == 'ymonmean' else month * 100 + day
    use = np.ones(key.shape, dtype=bool)
    if years is not None:
        y0, y1 = int(years[0]), int(years[1])
        use = (year >= y0) & (year <= y1)
    keys = np.unique(key[use]).astype(np.int64)
    bins = np.where(use, np.searchsorted(keys, key), -1).astype(np.int64) if len(keys) else np.full(key.shape, -1, dtype=np.int64)
    return keys, bins


def _clim_dtypes(in_dtype, out_dtype):
    dt = F32 if np.dtype(in_dtype) == F32 else F64
    odt = dt if out_dtype is None else np.dtype(out_dtype)
    if odt not in (F32, F64) or (odt == F32 and dt != F32):
        raise ValueError('out_dtype: the input dtype, or float64 for float32 input')
    return dt, odt


def _launch_clim(ctx, d_x, first, last, d_sum, d_cnt, d_mean, odt):
    """pgw_clim_accumulate over the records d_x (nrec, ...)."""
    inner = int(np.prod(d_x.shape[1:], dtype=np.int64))
    ctx._check(ctx.lib.pgw_clim_accumulate(ctx.handle, dtype_tag(d_x.dtype), dtype_tag(odt), d_x.shape[0], inner, d_x.ptr,
                                           1 if first else 0, 1 if last else 0, d_sum.ptr if d_sum is not None else None,
                                           d_cnt.ptr if d_cnt is not None else None, d_mean.ptr if d_mean is not None else None))


class _BinMean:
    """The mean of one bin after another through one chunk buffer of `nb` records: `fill(d_chunk, records)` puts the given
    records (indices into the series, time order) into the leading slots of the buffer, or returns another device array
    that already holds them.  A bin that fits the buffer is ONE launch with `first` and `last` both set and no accumulator
    in memory; a longer one goes through in chunks that carry sum / cnt on the device."""

    def __init__(self, ctx, rec_shape, dt, odt, nb):
        self.ctx, self.rec_shape, self.dt, self.odt, self.nb = ctx, tuple(rec_shape), dt, odt, int(nb)
        self.chunk = ctx.empty((self.nb,) + self.rec_shape, dt)
        self.sum = self.cnt = None

    def run(self, records, fill, d_mean):
        n = len(records)
        for r0 in range(0, n, self.nb):
            part = records[r0:r0 + self.nb]
            first, last = r0 == 0, r0 + len(part) == n
            if not (first and last) and self.sum is None:
                self.sum, self.cnt = self.ctx.empty(self.rec_shape, F64), self.ctx.empty(self.rec_shape, np.int32)
            d_x = fill(self.chunk, part)
            if d_x is None:
                d_x = self.chunk if len(part) == self.nb else DeviceArray(self.ctx, (len(part),) + self.rec_shape, self.dt,
                                                                         ptr=self.chunk.ptr, owner=self.chunk)
            _launch_clim(self.ctx, d_x, first, last, None if (first and last) else self.sum,
                         None if (first and last) else self.cnt, d_mean if last else None, self.odt)


def _records_of_bins(bin_of_record, nbin):
    b = np.asarray(bin_of_record).reshape(-1)
    if len(b) and (b.max() >= nbin or b.min() < -1):
        raise ValueError('bin_of_record must lie in [-1, nbin)')
    return [np.nonzero(b == k)[0] for k in range(int(nbin))]


def climatology(x, bin_of_record, nbin, out_dtype=None, max_records=None):
    """`cdo ymonmean` / `ydaymean` on arrays: x (time, ...) -> (nbin, ...), record k of the result the mean over the records
    r with bin_of_record[r] == k (`calendar_bins`), in time order, NaN = missing value skipped, float64 accumulation;
    cells without a sample (and bins without a record) are NaN.  Records with bin -1 are not read.
    out_dtype: the input's (default), or float64 for float32 input.  max_records caps the records per launch (a longer
    bin carries its sum on the device; the results do not depend on it).
    numpy, `ncio.Field` (labels re-wrapped, without the time coordinate) or `DeviceArray` in, the same kind out."""
    rx = raw(x)
    if len(rx.shape) < 1 or rx.shape[0] != len(np.asarray(bin_of_record).reshape(-1)):
        raise ValueError('bin_of_record must have one entry per record of x')
    nbin = int(nbin)
    if nbin < 1:
        raise ValueError('nbin must be positive')
    dt, odt = _clim_dtypes(rx.dtype, out_dtype)
    rec_shape = tuple(rx.shape[1:])
    inner = int(np.prod(rec_shape, dtype=np.int64))
    if inner < 1:
        raise ValueError('empty records')
    recs = _records_of_bins(bin_of_record, nbin)
    ctx = default_context()
    on_device = isinstance(rx, DeviceArray)
    if on_device and rx.dtype != dt:
        raise TypeError('device arrays must be float32 or float64, got %s' % rx.dtype)
    out = ctx.empty((nbin,) + rec_shape, odt)
    longest = max(len(r) for r in recs)
    if longest:
        nb = _fit_records(ctx, longest, inner * dt.itemsize, max_records)
        acc = _BinMean(ctx, rec_shape, dt, odt, nb)
        rec_bytes = inner * dt.itemsize
        host = None if on_device else np.empty((nb,) + rec_shape, dtype=dt)

        def fill(d_chunk, part):
            if on_device:
                if len(part) == 1 or np.all(np.diff(part) == 1):  # consecutive records: read where they are
                    return DeviceArray(ctx, (len(part),) + rec_shape, dt, ptr=rx.ptr + int(part[0]) * rec_bytes, owner=rx)
                for i, r in enumerate(part):
                    ctx._check(ctx.lib.pgw_memcpy_d2d(ctx.handle, d_chunk.ptr + i * rec_bytes, rx.ptr + int(r) * rec_bytes, rec_bytes))
                return None
            for i, r in enumerate(part):
                host[i] = rx[r]
            DeviceArray(ctx, (len(part),) + rec_shape, dt, ptr=d_chunk.ptr, owner=d_chunk).copy_from(host[:len(part)])
            return None
    nan_rec = None
    for k, part in enumerate(recs):
        if len(part):
            acc.run(part, fill, out.slab(k))
        else:
            nan_rec = np.full(rec_shape, np.nan, dtype=odt) if nan_rec is None else nan_rec
            out.slab(k).copy_from(nan_rec)
    if on_device:
        return out
    res = out.numpy()
    if is_labelled(x):
        dims = tuple(x.dims)
        coords = {d: v for d, v in getattr(x, 'coords', {}).items() if d in dims[1:]}
        return ncio.Field(res, dims, coords, dict(getattr(x, 'attrs', {})), getattr(x, 'name', None))
    return res


_FILL_KEYS = ('_FillValue', 'missing_value')
_PACK_KEYS = ('scale_factor', 'add_offset')


def _open_series(path, var_name):
    """(everything of the file but the variable's data, taken raw; a RecordReader of the variable)."""
    ds = ncio.open_dataset(path, decode_times=False, skip=(var_name,))
    if var_name not in ds:
        raise KeyError(var_name)
    return ds, ncio.RecordReader(path, var_name, decode_times=False)


def _time_axis(ds, reader, path):
    tdim = reader.dims[0]
    if tdim not in ds or 'units' not in ds[tdim].attrs:
        raise ValueError('%s: the first dimension %r has no coordinate with time units' % (path, tdim))
    t = ds[tdim]
    return tdim, np.asarray(t.values).reshape(-1), str(t.attrs['units']), str(t.attrs.get('calendar', 'standard'))


def _encoded(values, raw_attrs):
    """The decoded array as it goes into the file: NaN -> the input's `_FillValue` / `missing_value` when it has one
    (`ncio.to_netcdf` writes arrays as they are); the fill attributes in the array's dtype, packing attributes dropped
    (the values are the decoded ones)."""
    attrs = {k: v for k, v in raw_attrs.items() if k not in _PACK_KEYS}
    fill = None
    for k in _FILL_KEYS:
        if k in attrs:
            f = np.asarray(attrs[k]).reshape(-1)[0].astype(values.dtype)
            attrs[k] = f
            if fill is None and f == f:
                fill = f
    if fill is not None:
        values[np.isnan(values)] = fill
    return values, attrs


def climatology_files(inputs, out_path, var_name, mode, years=None, max_records=None, out_dtype=None):
    """extract_climate_delta.sh:194-219 without its `sellonlatbox`: `cdo -cat` of the files `inputs` (one path, or a list in
    time order - CMIP series come in multi-year pieces), `-selyear` (years=(y0, y1)), `ymonmean` / `ydaymean` (mode) of
    `var_name` -> `out_path`.
    The files must share the time units, the calendar and the record shape (ValueError).  Bin by bin (`calendar_bins`) the
    records are read in time order (`ncio.RecordReader`), uploaded in chunks of what fits into 80 % of the card's free
    memory, at most `max_records` (the results do not depend on it), and accumulated; records outside `years` are never
    read.  Output: the variable on (time = number of bins, ...) with the input's attributes in its decoded dtype
    (out_dtype='float64' widens a float32 series), every variable without the time dimension carried over, `time` = the raw
    time value of the LAST contributing record of each bin (cdo's convention for ymon* / yday*) with the input's units /
    calendar, records in key order.  Cells without a sample hold the input's `_FillValue` / `missing_value` (NaN if it has
    none).  NetCDF-3 in and out like everywhere in this package; the result loads through `functions.load_delta`."""
    if mode not in CLIM_MODES:
        raise ValueError('mode must be one of %s, got %r' % (CLIM_MODES, mode))
    paths = [inputs] if isinstance(inputs, (str, os.PathLike)) else list(inputs)
    if not paths:
        raise ValueError('no input file')
    opened = []
    try:
        for p in paths:
            opened.append(_open_series(p, var_name))
        ds0, r0 = opened[0]
        tdim, _, units, cal = _time_axis(ds0, r0, paths[0])
        times, where = [], []
        for k, (ds, rd) in enumerate(opened):
            td, t, u, c = _time_axis(ds, rd, paths[k])
            if (td, u, c.lower()) != (tdim, units, cal.lower()):
                raise ValueError('%s: time axis %r (%s, %s) differs from %r (%s, %s) of %s' % (paths[k], td, u, c, tdim, units, cal, paths[0]))
            if rd.rec_shape != r0.rec_shape or rd.dims != r0.dims or rd.dtype != r0.dtype:
                raise ValueError('%s: records %s %s %s differ from %s %s %s of %s'
                                 % (paths[k], rd.dims, rd.rec_shape, rd.dtype, r0.dims, r0.rec_shape, r0.dtype, paths[0]))
            if len(t) != rd.nrec:
                raise ValueError('%s: %d time values for %d records' % (paths[k], len(t), rd.nrec))
            times.append(t)
            where += [(k, i) for i in range(rd.nrec)]
        times = np.concatenate(times)
        keys, bins = calendar_bins(times, units, cal, mode, years)
        if not len(keys):
            raise ValueError('no record lies within the years %s' % (years,))
        dt, odt = _clim_dtypes(r0.dtype, out_dtype)
        rec_shape = r0.rec_shape
        inner = int(np.prod(rec_shape, dtype=np.int64))
        recs = _records_of_bins(bins, len(keys))
        ctx = default_context()
        nb = _fit_records(ctx, max(len(r) for r in recs), inner * dt.itemsize, max_records)
        acc = _BinMean(ctx, rec_shape, dt, odt, nb)
        host = np.empty((nb,) + rec_shape, dtype=dt)
        d_mean = ctx.empty(rec_shape, odt)
        result = np.empty((len(keys),) + rec_shape, dtype=odt)

        def fill(d_chunk, part):
            for i, r in enumerate(part):
                k, j = where[r]
                host[i] = opened[k][1].read_record(j)
            DeviceArray(ctx, (len(part),) + rec_shape, dt, ptr=d_chunk.ptr, owner=d_chunk).copy_from(host[:len(part)])

        for k, part in enumerate(recs):
            acc.run(part, fill, d_mean)
            result[k] = d_mean.numpy()
        t_out = np.array([times[part[-1]] for part in recs], dtype=times.dtype)
    finally:
        for _, rd in opened:
            rd.close()
    result, vattrs = _encoded(result, ds0[var_name].attrs)
    out = ncio.Dataset(attrs=dict(ds0.attrs), record_dim=ds0.record_dim)
    coords = {d: ds0[d].values for d in r0.dims[1:] if d in ds0}
    coords[tdim] = t_out
    for name, f in ds0.variables.items():
        if name == var_name:
            out[name] = ncio.Field(result, r0.dims, coords, vattrs)
        elif name == tdim:
            out[name] = ncio.Field(t_out, (tdim,), {tdim: t_out}, {k: v for k, v in f.attrs.items() if k != 'bounds'})
        elif tdim not in f.dims:
            out[name] = ncio.Field(f.values, f.dims, f.coords, dict(f.attrs))
    ncio.to_netcdf(out, out_path)
    return out_path


def _month_day_keys(ds, reader, path):
    tdim, t, units, cal = _time_axis(ds, reader, path)
    _, month, day = ncio.cf_year_month_day(t, units, cal)
    daily = len(np.unique(month)) < len(month)                    # several records per month: a day-of-year file
    return month, day, daily


def delta_files(scen_path, hist_path, out_path, var_name):
    """extract_climate_delta.sh:244-249, `cdo sub scenario historical delta`: the difference of two climatology files
    (`pgw_field_sub`, NaN / missing in either gives missing).  Both must have the same number of records, the same record
    shape and dtype and the same bin keys - the months of their time axes, and the days too in a day-of-year file -
    (ValueError).  Metadata and the time axis come from the scenario file, as cdo takes them from its first operand."""
    ds_s, rs = _open_series(scen_path, var_name)
    ds_h, rh = _open_series(hist_path, var_name)
    try:
        if rs.nrec != rh.nrec or rs.rec_shape != rh.rec_shape or rs.dtype != rh.dtype:
            raise ValueError('%s (%d records of %s %s) and %s (%d records of %s %s) do not match'
                             % (scen_path, rs.nrec, rs.rec_shape, rs.dtype, hist_path, rh.nrec, rh.rec_shape, rh.dtype))
        ms, dys, daily_s = _month_day_keys(ds_s, rs, scen_path)
        mh, dyh, daily_h = _month_day_keys(ds_h, rh, hist_path)
        if not np.array_equal(ms, mh) or daily_s != daily_h or (daily_s and not np.array_equal(dys, dyh)):
            raise ValueError('%s and %s do not hold the same months / days of the year' % (scen_path, hist_path))
        dt, _ = _clim_dtypes(rs.dtype, None)
        nrec, rec_shape = rs.nrec, rs.rec_shape
        inner = int(np.prod(rec_shape, dtype=np.int64))
        ctx = default_context()
        nb = _fit_records(ctx, nrec, 3 * inner * dt.itemsize)
        d_a, d_b, d_o = (ctx.empty((nb,) + rec_shape, dt) for _ in range(3))
        h_a, h_b = np.empty((nb,) + rec_shape, dtype=dt), np.empty((nb,) + rec_shape, dtype=dt)
        result = np.empty((nrec,) + rec_shape, dtype=dt)
        for r0 in range(0, nrec, nb):
            n = min(nb, nrec - r0)
            for i in range(n):
                h_a[i], h_b[i] = rs.read_record(r0 + i), rh.read_record(r0 + i)
            a, b, o = (DeviceArray(ctx, (n,) + rec_shape, dt, ptr=d.ptr, owner=d) for d in (d_a, d_b, d_o))
            a.copy_from(h_a[:n]); b.copy_from(h_b[:n])
            ctx._check(ctx.lib.pgw_field_sub(ctx.handle, dtype_tag(dt), n * inner, a.ptr, b.ptr, o.ptr))
            result[r0:r0 + n] = o.numpy()
    finally:
        rs.close(); rh.close()
    result, vattrs = _encoded(result, ds_s[var_name].attrs)
    out = ncio.Dataset(attrs=dict(ds_s.attrs), record_dim=ds_s.record_dim)
    for name, f in ds_s.variables.items():
        out[name] = ncio.Field(result, rs.dims, f.coords, vattrs) if name == var_name else ncio.Field(f.values, f.dims, f.coords, dict(f.attrs))
    ncio.to_netcdf(out, out_path)
    return out_path


def _parse_years(text):
    if text is None:
        return None
    parts = text.replace(',', '/').split('/')
    if len(parts) != 2:
        raise ValueError('years must be given as FIRST/LAST, e.g. 1985/2014')
    return int(parts[0]), int(parts[1])


# ------------------------------------------------------------------------------- command line
def build_parser():
    p = argparse.ArgumentParser(prog='python -m pgw4era5_amd.step_01_extract_deltas',
                                description='PGW for ERA5 step_01 on MI355X: CFday model levels to pressure levels, Emon hus to hur, '
                                            'climatologies and climate deltas.')
    sub = p.add_subparsers(dest='command', required=True)
    a = sub.add_parser('interp_to_plev', help='Interpolate CFday output to pressure levels (CFday_interp_to_plev.py)')
    a.add_argument('-i', '--input', type=str, required=True,
                   help='NetCDF-3 input file with the variable, ap, b (lev) and ps; {} is replaced by the variable name')
    a.add_argument('-o', '--output', type=str, required=True, help='output file; {} is replaced by the variable name')
    a.add_argument('-v', '--var_names', type=str, required=True, help='comma separated variable names, e.g. ta,hur,ua,va')
    a.add_argument('-p', '--target_p', type=str, required=True, help='text file with the target pressure levels in Pa')
    a.add_argument('-x', '--extrapolate', type=str, default='constant', choices=sorted(_lib.EXTRAP))
    a.add_argument('--max_records', type=int, default=None, help='at most this many time records per launch')
    a.add_argument('--out_dtype', type=str, default=None, choices=['float32', 'float64'])
    h = sub.add_parser('hus_to_hur', help='Convert GCM specific humidity to relative humidity (Emon_convert_hus_to_hur.py)')
    h.add_argument('hus_file', type=str)
    h.add_argument('ta_file', type=str)
    h.add_argument('hur_file', type=str)
    h.add_argument('-a', '--amon_hur_file', type=str, required=True, help='Amon relative humidity file')
    c = sub.add_parser('climatology', help='Multi-year monthly / day-of-year mean of a series (cdo -cat, -selyear, ymonmean / ydaymean)')
    c.add_argument('-i', '--input', type=str, required=True, nargs='+',
                   help='NetCDF-3 input files in time order; {} is replaced by the variable name')
    c.add_argument('-o', '--output', type=str, required=True, help='output file; {} is replaced by the variable name')
    c.add_argument('-v', '--var_names', type=str, required=True, help='comma separated variable names, e.g. ta,hur,ua,va')
    c.add_argument('-m', '--mode', type=str, required=True, choices=list(CLIM_MODES))
    c.add_argument('-y', '--years', type=str, default=None, help='first and last year to use, e.g. 1985/2014 (cdo selyear)')
    c.add_argument('--max_records', type=int, default=None, help='at most this many time records per launch')
    c.add_argument('--out_dtype', type=str, default=None, choices=['float32', 'float64'])
    d = sub.add_parser('delta', help='Scenario climatology minus historical climatology (cdo sub)')
    d.add_argument('scen_file', type=str, help='{} is replaced by the variable name (also in the other two paths)')
    d.add_argument('hist_file', type=str)
    d.add_argument('delta_file', type=str)
    d.add_argument('-v', '--var_names', type=str, required=True, help='comma separated variable names')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    done = []
    if args.command == 'interp_to_plev':
        names = args.var_names.split(',')
        if len(names) > 1 and ('{}' not in args.input or '{}' not in args.output):
            raise ValueError('several variables need {} in the input and the output path')
        for name in names:
            inp, out = args.input.replace('{}', name), args.output.replace('{}', name)
            print('Process input file: \n{}\nto output file: \n{}'.format(inp, out))
            done.append(interp_file(inp, out, name, args.target_p, extrapolate=args.extrapolate,
                                    max_records=args.max_records, out_dtype=args.out_dtype))
    elif args.command == 'hus_to_hur':
        done.append(hus_to_hur_file(args.hus_file, args.ta_file, args.hur_file, args.amon_hur_file))
    elif args.command == 'climatology':
        names = args.var_names.split(',')
        if len(names) > 1 and ('{}' not in args.output or not all('{}' in i for i in args.input)):
            raise ValueError('several variables need {} in the input and the output paths')
        years = _parse_years(args.years)
        for name in names:
            done.append(climatology_files([i.replace('{}', name) for i in args.input], args.output.replace('{}', name), name,
                                          args.mode, years=years, max_records=args.max_records, out_dtype=args.out_dtype))
    else:
        names = args.var_names.split(',')
        paths = (args.scen_file, args.hist_file, args.delta_file)
        if len(names) > 1 and not all('{}' in p for p in paths):
            raise ValueError('several variables need {} in all three paths')
        for name in names:
            done.append(delta_files(*[p.replace('{}', name) for p in paths], name))
    return done


if __name__ == '__main__':
    main()
