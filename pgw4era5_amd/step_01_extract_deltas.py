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

* `extract_climate_delta.sh:194-208`, `CFday_cut_subdomain.sh:28-30` (`cdo sellonlatbox,$box`) and
  `Emon_add_top_from_Amon.sh:45-56` (`cdo sellevel` twice, `cdo -O merge`): a level list, a latitude x cyclic-longitude
  window and the concatenation of two files' levels -> `lonlat_box` / `level_indices` / `select` / `select_file` /
  `merge_levels_files`, sub-commands `select` and `merge_levels`, and `climatology_files(box=...)`.  One kernel that moves
  words (`pgw_select_box`): the variable goes through the card as the raw bytes of the file, so its NetCDF type, fill
  values and packing are kept bit for bit.  Parity with cdo is unpinned here too; the docstrings are the contract.
  The ocean tables (`tos`, `siconc`, extract_climate_delta.sh:120-123) come on curvilinear grids with 2-D latitude /
  longitude: there the box is an index rectangle (`curvilinear_box`: the cells are marked on the card by
  `pgw_box_mark_2d`, the window found from the row and column flags), cut by the same kernel, coordinates unshifted.

The rest of the shell templates of step_01 (site paths, `wget`) are site scripts and stay out of scope (DESIGN.md
section 7).

Array kinds as in `functions.py`: numpy, `ncio.Field` (labels re-wrapped) or `DeviceArray` in, the same kind out.
Files are NetCDF-3 through `ncio` like everywhere in this package.
"""
import argparse
import os
import sys

import numpy as np

from . import _lib, ncio
from .device import DeviceArray, default_context, dtype_tag
from ._lib import _dp, _ip
from .operands import F32, F64, check_extrapolate, dev, is_labelled, out_like, raw
from .settings import LAT_GCM, LAT_GCM_OCEAN, LEV_GCM, LON_GCM, LON_GCM_OCEAN, PLEV_GCM, TIME_GCM

MAX_LEVELS = 256          # nsrc, ntarg, nplev limit of the kernels (include/pgw_hip.h)
COORD_PAIRS = ((LAT_GCM, LON_GCM), (LAT_GCM_OCEAN, LON_GCM_OCEAN))    # names of 2-D coordinates of a curvilinear grid


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


# ------------------------------------------------------------------------------- level list, lon-lat box, model-top merge
def lonlat_box(lat, lon, box):
    """`cdo sellonlatbox,lon1,lon2,lat1,lat2` on 1-D coordinates -> (lat0, nlat_sel, lon0, nlon_sel, lon_out): the rows
    lat0 .. lat0 + nlat_sel - 1 and the cyclic run of columns (lon0 + j) % len(lon), j < nlon_sel; `lon_out` their
    longitudes shifted into the box.
    box = (lon1, lon2, lat1, lat2) with lon1 < lon2 and lon2 - lon1 <= 360.  Rows with min(lat1, lat2) <= lat <= max(lat1,
    lat2) are kept in file order (north to south or south to north).  Column i is selected when lon1 <= lon[i] + 360 k <=
    lon2 for an integer k; the smallest such k is taken, so a column appears once, and the columns are ordered by that
    shifted longitude ascending - for the strictly ascending `lon` required here that is one cyclic run.  A box across 0
    deg on a 0 ... 360 grid (-73, 37) therefore gives negative, then positive longitudes; (0, 360, -90, 90) on a 0 ... <360
    grid is the identity.  ValueError: coordinates that are not 1-D (2-D curvilinear coordinates are not supported here),
    `lon` not strictly ascending, a bad box, rows that do not form one contiguous run (`lat` not monotonic), nothing
    selected."""
    lat, lon = np.asarray(raw(lat)), np.asarray(raw(lon))
    if lat.ndim != 1 or lon.ndim != 1:
        raise ValueError('lonlat_box needs 1-D lat and lon; 2-D (curvilinear) coordinates are not supported here')
    out_dtype = lon.dtype if lon.dtype.kind == 'f' else F64
    lat, lon = lat.astype(np.float64), lon.astype(np.float64)
    if len(lon) > 1 and not np.all(np.diff(lon) > 0):
        raise ValueError('lon must be strictly ascending')
    try:
        lon1, lon2, lat1, lat2 = (float(b) for b in box)
    except (TypeError, ValueError):
        raise ValueError('box must be (lon1, lon2, lat1, lat2), got %r' % (box,)) from None
    if not lon1 < lon2 or lon2 - lon1 > 360.0:
        raise ValueError('box needs lon1 < lon2 and lon2 - lon1 <= 360, got %r, %r' % (lon1, lon2))
    rows = np.nonzero((lat >= min(lat1, lat2)) & (lat <= max(lat1, lat2)))[0]
    if not len(rows):
        raise ValueError('no latitude lies within [%r, %r]' % (min(lat1, lat2), max(lat1, lat2)))
    if rows[-1] - rows[0] + 1 != len(rows):
        raise ValueError('the selected latitudes are not one contiguous run of rows: lat must be monotonic')
    k = np.ceil((lon1 - lon) / 360.0)                             # the smallest k with lon + 360 k >= lon1 ...
    k += (lon + 360.0 * k) < lon1                                 # ... whatever the division rounded to
    k -= (lon + 360.0 * (k - 1.0)) >= lon1
    shifted = lon + 360.0 * k
    cols = np.nonzero(shifted <= lon2)[0]
    if not len(cols):
        raise ValueError('no longitude lies within [%r, %r]' % (lon1, lon2))
    cols = cols[np.argsort(shifted[cols], kind='stable')]
    if not np.array_equal(cols, (cols[0] + np.arange(len(cols))) % len(lon)):
        raise ValueError('the selected longitudes are not one cyclic run of columns (does lon span more than 360 degrees?)')
    return int(rows[0]), int(len(rows)), int(cols[0]), int(len(cols)), shifted[cols].astype(out_dtype)


def _box_values(box):
    """(lon1, lon2, lat1, lat2) as floats with the checks of `lonlat_box`."""
    try:
        lon1, lon2, lat1, lat2 = (float(b) for b in box)
    except (TypeError, ValueError):
        raise ValueError('box must be (lon1, lon2, lat1, lat2), got %r' % (box,)) from None
    if lat1 != lat1 or lat2 != lat2:
        raise ValueError('box must not hold a NaN, got %r' % (box,))
    if not lon1 < lon2 or lon2 - lon1 > 360.0:
        raise ValueError('box needs lon1 < lon2 and lon2 - lon1 <= 360, got %r, %r' % (lon1, lon2))
    return lon1, lon2, lat1, lat2


CYCLIC_CHOICES = {'auto': 'auto', 'yes': True, 'no': False}


def _check_cyclic(cyclic):
    if isinstance(cyclic, str) and cyclic in CYCLIC_CHOICES:
        return CYCLIC_CHOICES[cyclic]
    if cyclic is True or cyclic is False:
        return cyclic
    raise ValueError("cyclic must be 'auto', True or False, got %r" % (cyclic,))


def _chord(lat_a, lon_a, lat_b, lon_b):
    """Chord length on the unit sphere between two lists of points in degrees."""
    def xyz(lat, lon):
        la, lo = np.deg2rad(lat), np.deg2rad(lon)
        return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    return np.sqrt(np.sum((xyz(lat_a, lon_a) - xyz(lat_b, lon_b)) ** 2, axis=0))


def grid_is_cyclic(lat2d, lon2d):
    """Does the curvilinear grid (nj, ni) close on itself along i?  Decided from three cells at each end of every row whose
    four end cells (columns 0, 1, ni - 2, ni - 1) are finite: the row votes yes when the chord from its last cell to its
    first is at most 1.5 times the longer of its first and last cell-to-cell chords; the grid is cyclic when more than half
    of those rows vote yes.  ni < 3, or no such row: not cyclic.  A global grid is cyclic, with or without duplicated halo
    columns at its ends (NEMO, MPI-ESM); a regional or rotated-pole grid is not."""
    lat, lon = np.asarray(lat2d, dtype=np.float64), np.asarray(lon2d, dtype=np.float64)
    if lat.ndim != 2 or lat.shape != lon.shape:
        raise ValueError('lat2d and lon2d must be 2-D arrays of one shape, got %s and %s' % (lat.shape, lon.shape))
    ni = lat.shape[1]
    if ni < 3:
        return False
    ends = [0, 1, ni - 2, ni - 1]
    ok = np.all(np.isfinite(lat[:, ends]) & np.isfinite(lon[:, ends]), axis=1)
    if not np.any(ok):
        return False
    la, lo = lat[ok], lon[ok]
    seam = _chord(la[:, ni - 1], lo[:, ni - 1], la[:, 0], lo[:, 0])
    step = np.maximum(_chord(la[:, 0], lo[:, 0], la[:, 1], lo[:, 1]), _chord(la[:, ni - 2], lo[:, ni - 2], la[:, ni - 1], lo[:, ni - 1]))
    return bool(2 * int(np.count_nonzero(seam <= 1.5 * step)) > len(seam))


def flag_windows(row_any, col_any, cyclic):
    """The index rectangle of the flags of `pgw_box_mark_2d` -> (j0, nj_sel, i0, ni_sel).
    Rows: first flagged row to last flagged row, unflagged rows between them kept.  Columns of a grid that is not cyclic:
    the same.  Columns of a cyclic grid: the complement of the longest cyclic run of unflagged columns (a tie goes to the
    run that starts at the lowest index), as the cyclic run (i0 + c) % ni, c < ni_sel, that `pgw_select_box` takes; all
    columns flagged gives (0, ni).  ValueError: no flagged row or column."""
    rows, cols = np.nonzero(np.asarray(row_any).reshape(-1))[0], np.asarray(col_any).reshape(-1) != 0
    ni = len(cols)
    on = np.nonzero(cols)[0]
    if not len(rows) or not len(on):
        raise ValueError('no row or column is flagged')
    j0, nj_sel = int(rows[0]), int(rows[-1] - rows[0] + 1)
    if not cyclic:
        return j0, nj_sel, int(on[0]), int(on[-1] - on[0] + 1)
    if len(on) == ni:
        return j0, nj_sel, 0, ni
    # an unflagged run starts behind every flagged column that is followed by an unflagged one and lasts up to the next
    # flagged column (cyclically)
    nxt = np.concatenate([on[1:], on[:1] + ni])
    length = nxt - on - 1
    start = (on + 1) % ni
    best = np.lexsort((start, -length))[0]                         # longest, then the lowest start
    return j0, nj_sel, int((start[best] + length[best]) % ni), int(ni - length[best])


def curvilinear_box(lat2d, lon2d, box, cyclic='auto'):
    """`cdo sellonlatbox,lon1,lon2,lat1,lat2` on a curvilinear grid with 2-D coordinates lat2d, lon2d (nj, ni), float32 or
    float64 in degrees (extract_climate_delta.sh:120-123, 194-208: the Omon / SImon tables) -> (j0, nj_sel, i0, ni_sel,
    n_inside): the index rectangle of rows j0 .. j0 + nj_sel - 1 and the run of columns (i0 + c) % ni, c < ni_sel, that holds
    every cell inside the box; the output stays curvilinear and its coordinates keep their bits (no 360 k shift).
    box as in `lonlat_box`.  A cell is inside when its coordinates are finite, min(lat1, lat2) <= lat <= max(lat1, lat2)
    and lon1 <= lon + 360 k <= lon2 for an integer k (the smallest k with lon + 360 k >= lon1 is tried; edges inclusive;
    float64 arithmetic).  The cells are marked on the card (`pgw_box_mark_2d`); the rectangle is found on the host from the
    nj + ni flags (`flag_windows`).  Cells of the rectangle that lie outside the box are kept, as cdo keeps them.
    cyclic: does the grid close on itself along i - 'auto' (`grid_is_cyclic`), True or False.  On a cyclic grid a box
    across the seam gives a short run of columns that wraps; on any other grid first to last flagged column.
    ValueError: a bad box, coordinates that are not 2-D arrays of one shape, no cell inside the box."""
    lon1, lon2, lat1, lat2 = _box_values(box)
    cyclic = _check_cyclic(cyclic)
    rla, rlo = raw(lat2d), raw(lon2d)
    rla = rla.numpy() if isinstance(rla, DeviceArray) else np.asarray(rla)
    rlo = rlo.numpy() if isinstance(rlo, DeviceArray) else np.asarray(rlo)
    if rla.ndim != 2 or rla.shape != rlo.shape or rla.size < 1:
        raise ValueError('lat2d and lon2d must be 2-D arrays of one shape, got %s and %s' % (rla.shape, rlo.shape))
    dt = F32 if (rla.dtype == F32 and rlo.dtype == F32) else F64
    nj, ni = rla.shape
    if cyclic == 'auto':
        cyclic = grid_is_cyclic(rla, rlo)
    ctx = default_context()
    d_lat, d_lon = dev(ctx, rla, dt), dev(ctx, rlo, dt)
    d_out = ctx.empty((2 + nj + ni,), np.int32)                     # n_inside (8 bytes), row_any, col_any
    ctx._check(ctx.lib.pgw_box_mark_2d(ctx.handle, dtype_tag(dt), nj, ni, d_lat.ptr, d_lon.ptr, lon1, lon2, lat1, lat2,
                                       d_out.ptr + 8, d_out.ptr + 8 + 4 * nj, d_out.ptr))
    flags = d_out.numpy()
    n_inside = int(flags[:2].view(np.int64)[0])
    if n_inside == 0:
        raise ValueError('no cell lies within the box %r' % ((lon1, lon2, lat1, lat2),))
    return flag_windows(flags[2:2 + nj], flags[2 + nj:], cyclic) + (n_inside,)


def level_indices(plev, levels):
    """`cdo sellevel,levels`: the indices into `plev` of the requested values IN FILE ORDER (cdo keeps the file's order
    whatever the order of the request).  Exact equality.  ValueError: a requested level that is absent (named), a level
    requested twice."""
    plev = np.asarray(raw(plev)).astype(np.float64).reshape(-1)
    want = np.atleast_1d(np.asarray(levels, dtype=np.float64)).reshape(-1)
    if not len(want):
        raise ValueError('no level requested')
    for i, v in enumerate(want):
        if not np.any(plev == v):
            raise ValueError('level %r is not in the file (levels: %s)' % (float(v), plev.tolist()))
        if np.any(want[:i] == v):
            raise ValueError('level %r is requested twice' % float(v))
    return np.nonzero(np.isin(plev, want))[0].astype(np.int32)


def _launch_select(ctx, itemsize, nrec, nlev_src, nlat_src, nlon_src, src_ptr, lev_idx, rows, cols, nlev_dst, lev_dst0, dst_ptr):
    """pgw_select_box: lev_idx (int array, or None = all nlev_src levels), rows = (lat0, nlat_sel), cols = (lon0, nlon_sel)."""
    if lev_idx is None:
        nsel, p_lev = nlev_src, None
    else:
        lev_idx = np.ascontiguousarray(lev_idx, dtype=np.int32)
        nsel, p_lev = len(lev_idx), lev_idx.ctypes.data_as(_ip)
    ctx._check(ctx.lib.pgw_select_box(ctx.handle, int(itemsize), int(nrec), int(nlev_src), int(nlat_src), int(nlon_src), src_ptr,
                                      int(nsel), p_lev, int(rows[0]), int(rows[1]), int(cols[0]), int(cols[1]), int(nlev_dst),
                                      int(lev_dst0), dst_ptr))


def _upload_words(ctx, d, host):
    """host -> the DeviceArray d as it is: no cast and no byte-order conversion (`DeviceArray.copy_from` converts)."""
    host = np.ascontiguousarray(host)
    if host.nbytes != d.nbytes:
        raise ValueError('upload of %d bytes into a device array of %d' % (host.nbytes, d.nbytes))
    if d.nbytes:
        ctx._check(ctx.lib.pgw_memcpy_h2d(ctx.handle, d.ptr, host.ctypes.data, d.nbytes))
        ctx.sync()                                                # pageable source


def _word_size(dtype):
    n = np.dtype(dtype).itemsize
    if n not in (2, 4, 8):
        raise ValueError('elements of 2, 4 or 8 bytes (NetCDF short, int / float, double) can be selected, got %s' % np.dtype(dtype))
    return n


def _coord_pair_2d(coords, shape2):
    """The names of a pair of 2-D coordinates of shape `shape2` among `coords` (name -> array), or None."""
    for la, lo in COORD_PAIRS:
        if la in coords and lo in coords and np.shape(raw(coords[la])) == np.shape(raw(coords[lo])) == tuple(shape2) and len(shape2) == 2:
            return la, lo
    return None


def select(field, levels=None, box=None, plev=None, lat=None, lon=None, cyclic='auto'):
    """`cdo sellevel` and / or `cdo sellonlatbox` on an array (..., [plev,] lat, lon): a numpy array, an `ncio.Field` or a
    `DeviceArray` in, the same kind and the same dtype out (elements of 2, 4 or 8 bytes are moved as words, any byte
    order).  levels: the level values to keep (`level_indices`, file order); box = (lon1, lon2, lat1, lat2)
    (`lonlat_box`).  plev / lat / lon: the 1-D coordinates; a labelled input brings its own and comes back with the cut /
    shifted ones.  The array has a level axis - third from the end - when `plev` is given or a labelled input names it.
    A curvilinear grid: `lat` and `lon` are 2-D arrays of the shape of the last two axes (..., [plev,] j, i) - given, or
    found among a labelled input's coordinates under the names lat / lon or latitude / longitude.  The box then selects
    the index rectangle of `curvilinear_box` (`cyclic` as there; anything but 'auto' is a ValueError with 1-D
    coordinates); a labelled input comes back with its 2-D coordinates cut, bits kept."""
    cyclic = _check_cyclic(cyclic)
    r = raw(field)
    shape = tuple(r.shape)
    labelled = is_labelled(field)
    coords = dict(getattr(field, 'coords', {})) if labelled else {}
    dims = tuple(field.dims) if labelled else None
    pair = None
    if labelled and lat is None and lon is None and len(shape) >= 2:
        pair = _coord_pair_2d(coords, shape[-2:])
        if pair is not None:
            lat, lon = coords[pair[0]], coords[pair[1]]
    curv = lat is not None and lon is not None and np.ndim(raw(lat)) == 2 and np.ndim(raw(lon)) == 2
    if labelled:
        if len(dims) < 2 or (dims[-2:] != (LAT_GCM, LON_GCM) and not curv):
            raise ValueError('the dimensions must end in ([%s,] %s, %s), got %s' % (PLEV_GCM, LAT_GCM, LON_GCM, dims))
        has_lev = len(dims) >= 3 and dims[-3] == PLEV_GCM
        plev = coords.get(PLEV_GCM) if plev is None and has_lev else plev
        if not curv:
            lat = coords.get(LAT_GCM) if lat is None else lat
            lon = coords.get(LON_GCM) if lon is None else lon
    else:
        has_lev = plev is not None
    if not curv and cyclic != 'auto':
        raise ValueError('cyclic applies to 2-D (curvilinear) coordinates only; with 1-D lat / lon it must be auto')
    if len(shape) < (3 if has_lev else 2):
        raise ValueError('expected an array (..., %slat, lon), got shape %s' % ('plev, ' if has_lev else '', shape))
    nlat, nlon = shape[-2:]
    nlev = shape[-3] if has_lev else 1
    lev_idx, rows, cols, lon_out = None, (0, nlat), (0, nlon), None
    if levels is not None:
        if not has_lev or plev is None:
            raise ValueError('levels need an array with a level axis and its plev coordinate')
        if len(np.asarray(raw(plev)).reshape(-1)) != nlev:
            raise ValueError('plev has %d values for %d levels' % (len(np.asarray(raw(plev)).reshape(-1)), nlev))
        lev_idx = level_indices(plev, levels)
    if box is not None:
        if lat is None or lon is None:
            raise ValueError('a box needs the lat and lon coordinates')
        if curv:
            if np.shape(raw(lat)) != (nlat, nlon) or np.shape(raw(lon)) != (nlat, nlon):
                raise ValueError('2-D lat / lon do not match the last two axes %s' % ((nlat, nlon),))
            lat0, nlat_sel, lon0, nlon_sel, _ = curvilinear_box(lat, lon, box, cyclic)
        else:
            if np.shape(raw(lat)) != (nlat,) or np.shape(raw(lon)) != (nlon,):
                raise ValueError('lat / lon do not match the last two axes %s' % ((nlat, nlon),))
            lat0, nlat_sel, lon0, nlon_sel, lon_out = lonlat_box(lat, lon, box)
        rows, cols = (lat0, nlat_sel), (lon0, nlon_sel)
    item = _word_size(r.dtype)
    lead = shape[:-3] if has_lev else shape[:-2]
    nrec = int(np.prod(lead, dtype=np.int64))
    nsel = nlev if lev_idx is None else len(lev_idx)
    out_shape = lead + ((nsel,) if has_lev else ()) + (rows[1], cols[1])
    if nrec < 1:
        raise ValueError('empty array')
    ctx = default_context()
    if isinstance(r, DeviceArray):
        d_in = r
    else:
        d_in = ctx.empty(shape, r.dtype)
        _upload_words(ctx, d_in, r)
    d_out = ctx.empty(out_shape, r.dtype)
    _launch_select(ctx, item, nrec, nlev, nlat, nlon, d_in.ptr, lev_idx, rows, cols, nsel, 0, d_out.ptr)
    if isinstance(r, DeviceArray):
        return d_out
    host = d_out.numpy()
    if not labelled:
        return host
    if lev_idx is not None:
        coords[PLEV_GCM] = np.asarray(raw(plev)).reshape(-1)[lev_idx]
    if box is not None and curv:
        jj, ii = slice(rows[0], rows[0] + rows[1]), (cols[0] + np.arange(cols[1])) % nlon
        for d, idx in ((dims[-2], jj), (dims[-1], ii)):           # 1-D index coordinates of the two grid dimensions
            if d in coords and np.ndim(coords[d]) == 1:
                coords[d] = np.asarray(coords[d])[idx]
        if pair is not None:
            for name in pair:
                coords[name] = np.asarray(raw(coords[name]))[jj][:, ii]
    elif box is not None:
        coords[LAT_GCM] = np.asarray(raw(lat))[rows[0]:rows[0] + rows[1]]
        coords[LON_GCM] = lon_out
    return ncio.Field(host, dims, coords, dict(getattr(field, 'attrs', {})), getattr(field, 'name', None))


def _curvilinear_pair(ds, dims):
    """The names (lat, lon) of the pair of 2-D coordinate variables of the file whose dimensions are exactly the last two
    of `dims` - the variable is on a curvilinear grid - or None."""
    dims = tuple(dims)
    if len(dims) >= 2:
        for la, lo in COORD_PAIRS:
            if la in ds and lo in ds and tuple(ds[la].dims) == tuple(ds[lo].dims) == dims[-2:]:
                return la, lo
    return None


class _Cut:
    """What a selection does to every OTHER variable of a file, on the host: the level indices along `plev`, the rows along
    `lat`, the cyclic run of columns along `lon`; the longitude coordinate and its bounds take the +360 k shift.
    `dims`: the dimensions of the selected variable.  When the file holds 2-D coordinates on its last two dimensions
    (`_curvilinear_pair`) the box is the index rectangle of `curvilinear_box`: the row run and the cyclic column run go along
    those two grid dimensions - through the 2-D coordinates and `vertices_latitude` / `vertices_longitude` too - and nothing
    is shifted."""

    def __init__(self, ds, lev_idx=None, box=None, dims=None, cyclic='auto'):
        self.lev_idx = None if lev_idx is None else np.asarray(lev_idx, dtype=np.int64)
        self.rows = self.cols = self.shift = None
        self.lon_names = ()
        self.row_dim, self.col_dim = LAT_GCM, LON_GCM
        cyclic = _check_cyclic(cyclic)
        pair = _curvilinear_pair(ds, dims) if (box is not None and dims is not None) else None
        if pair is None and cyclic != 'auto':
            raise ValueError('cyclic applies to 2-D (curvilinear) coordinates only; with 1-D lat / lon it must be auto')
        if pair is not None:
            self.row_dim, self.col_dim = tuple(dims)[-2:]
            lat, lon = ds[pair[0]].values, ds[pair[1]].values
            self.lat0, self.nlat_sel, self.lon0, self.nlon_sel, _ = curvilinear_box(lat, lon, box, cyclic)
            self.rows = slice(self.lat0, self.lat0 + self.nlat_sel)
            self.cols = (self.lon0 + np.arange(self.nlon_sel)) % np.shape(lon)[1]
        elif box is not None:
            for d in (LAT_GCM, LON_GCM):
                if d not in ds:
                    raise ValueError('a box needs the coordinate variable %s in the file' % d)
            lat, lon = ds[LAT_GCM].values, ds[LON_GCM].values
            self.lat0, self.nlat_sel, self.lon0, self.nlon_sel, lon_out = lonlat_box(lat, lon, box)
            self.rows = slice(self.lat0, self.lat0 + self.nlat_sel)
            self.cols = (self.lon0 + np.arange(self.nlon_sel)) % len(lon)
            self.shift = np.round((lon_out.astype(np.float64) - np.asarray(lon, dtype=np.float64)[self.cols]) / 360.0) * 360.0
            self.lon_names = (LON_GCM, str(ds[LON_GCM].attrs.get('bounds', LON_GCM + '_bnds')))

    def touches(self, f):
        return ((self.lev_idx is not None and PLEV_GCM in f.dims) or
                (self.rows is not None and (self.row_dim in f.dims or self.col_dim in f.dims)))

    def field(self, name, f):
        """The variable `f` of the input cut with the selection's indices."""
        if not self.touches(f):
            return ncio.Field(f.values, f.dims, f.coords, dict(f.attrs))
        v = np.asarray(f.values)
        for ax, d in enumerate(f.dims):
            if d == PLEV_GCM and self.lev_idx is not None:
                v = np.take(v, self.lev_idx, axis=ax)
            elif d == self.row_dim and self.rows is not None:
                v = v[(slice(None),) * ax + (self.rows,)]
            elif d == self.col_dim and self.cols is not None:
                v = np.take(v, self.cols, axis=ax)
                if name in self.lon_names and v.dtype.kind == 'f':
                    sh = self.shift.reshape((-1,) + (1,) * (v.ndim - ax - 1))
                    v = np.where(sh != 0, v + sh, v).astype(v.dtype)           # columns that do not move keep their bits
        return ncio.Field(v, f.dims, {}, dict(f.attrs))


def _grid_dims(dims, what, ds=None):
    """(number of leading dimensions, has a level axis) of a variable whose dimensions end in ([plev,] lat, lon) - or, with
    the file `ds` given, in ([plev,] j, i) of a curvilinear grid (`_curvilinear_pair`)."""
    dims = tuple(dims)
    curv = ds is not None and _curvilinear_pair(ds, dims) is not None
    if len(dims) < 2 or (dims[-2:] != (LAT_GCM, LON_GCM) and not curv):
        raise ValueError('%s: the dimensions must end in ([%s,] %s, %s), got %s' % (what, PLEV_GCM, LAT_GCM, LON_GCM, dims))
    has_lev = len(dims) >= 3 and dims[-3] == PLEV_GCM
    nlead = len(dims) - (3 if has_lev else 2)
    if nlead < 1:
        raise ValueError('%s: a leading (time) dimension is needed in front of ([%s,] %s, %s), got %s'
                         % (what, PLEV_GCM, LAT_GCM, LON_GCM, dims))
    return nlead, has_lev


class _RawChunks:
    """The records of one variable as raw file words through one device buffer of `nb` records: `load(r0, n)` reads records
    r0 .. r0 + n - 1 (`RecordReader.read_record_raw`) and uploads them as they are; -> the device pointer."""

    def __init__(self, ctx, reader, nb):
        self.ctx, self.reader = ctx, reader
        big = reader.file_dtype.newbyteorder('>')
        self.host = np.empty((nb,) + reader.rec_shape, dtype=big)
        self.dev = ctx.empty((nb,) + reader.rec_shape, big)

    def load(self, r0, n):
        for i in range(n):
            self.reader.read_record_raw(r0 + i, out=self.host[i])
        part = DeviceArray(self.ctx, (n,) + self.reader.rec_shape, self.host.dtype, ptr=self.dev.ptr, owner=self.dev)
        _upload_words(self.ctx, part, self.host[:n])
        return self.dev.ptr


def select_file(inp, out, var_name, levels=None, box=None, max_records=None, cyclic='auto'):
    """`cdo sellevel,levels` and / or `cdo sellonlatbox,box` of one NetCDF-3 file (CFday_cut_subdomain.sh:28-30,
    extract_climate_delta.sh:194-208, Emon_add_top_from_Amon.sh:45-52) -> `out`.
    `var_name`, on (time, ..., [plev,] lat, lon) as named by settings, goes through the card in chunks of records
    (`ncio.RecordReader`, what fits into 80 % of the free memory, at most `max_records`; the result does not depend on it)
    AS THE RAW WORDS OF THE FILE: the output variable keeps its NetCDF type, every attribute, `_FillValue` and packing, and
    its bytes are the input's.  Every other variable with the level, latitude or longitude dimension - the coordinates,
    `lat_bnds`, `lon_bnds`, `plev_bnds` - is cut on the host with the same indices, `lon` and its bounds variable shifted by
    the same 360 k (`lonlat_box`); everything else, the global attributes and the record dimension are carried over.
    A curvilinear file (extract_climate_delta.sh:120-123, the Omon / SImon tables): when the file holds 2-D coordinate
    variables lat / lon or latitude / longitude whose dimensions are exactly the variable's last two, (..., [plev,] j, i),
    the box selects the index rectangle of `curvilinear_box` (`cyclic` as there) and every other variable on either grid
    dimension - the 2-D coordinates, `vertices_latitude` / `vertices_longitude` - is cut with the same row run and cyclic
    column run; no longitude is shifted, the coordinates keep their bits.  With 1-D coordinates `cyclic` must be 'auto'."""
    ds, rd = _open_series(inp, var_name)
    try:
        nlead, has_lev = _grid_dims(rd.dims, var_name, ds)
        item = _word_size(rd.file_dtype)
        lev_idx = None
        if levels is not None:
            if not has_lev or PLEV_GCM not in ds:
                raise ValueError('%s: levels need the %s dimension and its coordinate variable' % (var_name, PLEV_GCM))
            lev_idx = level_indices(ds[PLEV_GCM].values, levels)
        cut = _Cut(ds, lev_idx, box, rd.dims, cyclic)
        nrec, rec_shape = rd.nrec, rd.rec_shape
        nlat, nlon = rec_shape[-2:]
        nlev = rec_shape[-3] if has_lev else 1
        fold = int(np.prod(rec_shape[:nlead - 1], dtype=np.int64))          # leading dimensions behind the first one
        rows = (cut.lat0, cut.nlat_sel) if box is not None else (0, nlat)
        cols = (cut.lon0, cut.nlon_sel) if box is not None else (0, nlon)
        nsel = nlev if lev_idx is None else len(lev_idx)
        out_rec = rec_shape[:nlead - 1] + ((nsel,) if has_lev else ()) + (rows[1], cols[1])
        big = rd.file_dtype.newbyteorder('>')
        ctx = default_context()
        per_rec = (int(np.prod(rec_shape, dtype=np.int64)) + int(np.prod(out_rec, dtype=np.int64))) * item
        nb = _fit_records(ctx, nrec, per_rec, max_records)
        chunks = _RawChunks(ctx, rd, nb)
        d_out = ctx.empty((nb,) + out_rec, big)
        result = np.empty((nrec,) + out_rec, dtype=big)
        for r0 in range(0, nrec, nb):
            n = min(nb, nrec - r0)
            src = chunks.load(r0, n)
            _launch_select(ctx, item, n * fold, nlev, nlat, nlon, src, lev_idx, rows, cols, nsel, 0, d_out.ptr)
            result[r0:r0 + n] = DeviceArray(ctx, (n,) + out_rec, big, ptr=d_out.ptr, owner=d_out).numpy()
    finally:
        rd.close()
    res = ncio.Dataset(attrs=dict(ds.attrs), record_dim=ds.record_dim)
    for name, f in ds.variables.items():
        res[name] = ncio.Field(result, rd.dims, {}, dict(rd.file_attrs)) if name == var_name else cut.field(name, f)
    ncio.to_netcdf(res, out)
    return out


def merge_levels_files(path_a, path_b, out, var_name, levels_a=None, levels_b=None, max_records=None):
    """Emon_add_top_from_Amon.sh:45-56 in one go - `cdo sellevel,levels_a a`, `cdo sellevel,levels_b b`, `cdo -O merge` -
    without the two intermediate files: `var_name` of `out` holds the (selected, file order) levels of `path_a`, then those
    of `path_b`, two `pgw_select_box` launches per chunk of records into one destination, raw file words as in
    `select_file`.  levels_* = None: all levels of that file.
    ValueError: the two variables are not on the same (time, ..., plev, lat, lon) dimensions and record shapes apart from the
    number of levels, their time / lat / lon coordinates differ (the rule of `merge_hur_levels`: nothing is aligned), their
    NetCDF types differ, a level is in both selections.  Metadata - global attributes, the variable's and the level
    coordinate's attributes, every other variable - come from `path_a`; the level coordinate, and its bounds variable when
    both files have it, are concatenated; other variables of `path_a` on the level dimension are left out.  The result
    loads through `functions.load_delta`."""
    ds_a, ra = _open_series(path_a, var_name)
    try:
        ds_b, rb = _open_series(path_b, var_name)
    except Exception:
        ra.close()
        raise
    try:
        what = 'merge_levels_files'
        for ds, rd, p in ((ds_a, ra, path_a), (ds_b, rb, path_b)):
            nlead, has_lev = _grid_dims(rd.dims, '%s of %s' % (var_name, p))
            if not has_lev or PLEV_GCM not in ds:
                raise ValueError('%s of %s has no %s dimension with a coordinate variable' % (var_name, p, PLEV_GCM))
        if ra.dims != rb.dims or ra.nrec != rb.nrec or ra.rec_shape[:-3] + ra.rec_shape[-2:] != rb.rec_shape[:-3] + rb.rec_shape[-2:]:
            raise ValueError('%s: %s %s (%d records) of %s and %s %s (%d records) of %s do not match'
                             % (what, ra.dims, ra.rec_shape, ra.nrec, path_a, rb.dims, rb.rec_shape, rb.nrec, path_b))
        _same_coords(ds_a[var_name], ds_b[var_name], what)
        if ra.file_dtype != rb.file_dtype:
            raise ValueError('%s: the NetCDF types differ: %s in %s, %s in %s' % (what, ra.file_dtype, path_a, rb.file_dtype, path_b))
        item = _word_size(ra.file_dtype)
        plev_a, plev_b = np.asarray(ds_a[PLEV_GCM].values).reshape(-1), np.asarray(ds_b[PLEV_GCM].values).reshape(-1)
        ia = np.arange(len(plev_a), dtype=np.int32) if levels_a is None else level_indices(plev_a, levels_a)
        ib = np.arange(len(plev_b), dtype=np.int32) if levels_b is None else level_indices(plev_b, levels_b)
        both = np.intersect1d(plev_a[ia].astype(np.float64), plev_b[ib].astype(np.float64))
        if len(both):
            raise ValueError('%s: levels %s are selected from both files' % (what, both.tolist()))
        nlev_out = len(ia) + len(ib)
        if nlev_out > MAX_LEVELS:
            raise ValueError('%s: at most %d levels, got %d' % (what, MAX_LEVELS, nlev_out))
        nrec, nlat, nlon = ra.nrec, ra.rec_shape[-2], ra.rec_shape[-1]
        fold = int(np.prod(ra.rec_shape[:-3], dtype=np.int64))
        out_rec = ra.rec_shape[:-3] + (nlev_out, nlat, nlon)
        big = ra.file_dtype.newbyteorder('>')
        ctx = default_context()
        per_rec = sum(int(np.prod(s, dtype=np.int64)) for s in (ra.rec_shape, rb.rec_shape, out_rec)) * item
        nb = _fit_records(ctx, nrec, per_rec, max_records)
        ca, cb = _RawChunks(ctx, ra, nb), _RawChunks(ctx, rb, nb)
        d_out = ctx.empty((nb,) + out_rec, big)
        result = np.empty((nrec,) + out_rec, dtype=big)
        for r0 in range(0, nrec, nb):
            n = min(nb, nrec - r0)
            src_a, src_b = ca.load(r0, n), cb.load(r0, n)
            _launch_select(ctx, item, n * fold, len(plev_a), nlat, nlon, src_a, ia, (0, nlat), (0, nlon), nlev_out, 0, d_out.ptr)
            _launch_select(ctx, item, n * fold, len(plev_b), nlat, nlon, src_b, ib, (0, nlat), (0, nlon), nlev_out, len(ia), d_out.ptr)
            result[r0:r0 + n] = DeviceArray(ctx, (n,) + out_rec, big, ptr=d_out.ptr, owner=d_out).numpy()
    finally:
        ra.close(); rb.close()
    bnds = str(ds_a[PLEV_GCM].attrs.get('bounds', PLEV_GCM + '_bnds'))
    res = ncio.Dataset(attrs=dict(ds_a.attrs), record_dim=ds_a.record_dim)
    for name, f in ds_a.variables.items():
        if name == var_name:
            res[name] = ncio.Field(result, ra.dims, {}, dict(ra.file_attrs))
        elif name == PLEV_GCM or (name == bnds and name in ds_b and f.dims and f.dims[0] == PLEV_GCM and ds_b[name].dims == f.dims):
            v = np.concatenate([np.asarray(f.values)[ia], np.asarray(ds_b[name].values)[ib].astype(f.values.dtype)])
            res[name] = ncio.Field(v, f.dims, {}, dict(f.attrs))
        elif PLEV_GCM not in f.dims:
            res[name] = ncio.Field(f.values, f.dims, {}, dict(f.attrs))
    if bnds not in res and 'bounds' in res[PLEV_GCM].attrs:
        del res[PLEV_GCM].attrs['bounds']
    ncio.to_netcdf(res, out)
    return out


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


def climatology_files(inputs, out_path, var_name, mode, years=None, max_records=None, out_dtype=None, box=None, cyclic='auto'):
    """extract_climate_delta.sh:194-219: `cdo -cat` of the files `inputs` (one path, or a list in
    time order - CMIP series come in multi-year pieces), `-selyear` (years=(y0, y1)), `ymonmean` / `ydaymean` (mode) of
    `var_name` -> `out_path`.
    box = (lon1, lon2, lat1, lat2): the `sellonlatbox,$box` in front of it (:194, :204; `lonlat_box`) - every uploaded chunk
    of decoded records is cut on the device (`pgw_select_box`) before it is accumulated, the dimensions must end in
    ([plev,] lat, lon), and the coordinates and bounds of the output are cut as `select_file` cuts them: the result is, bit
    for bit, the climatology of the `select_file(box=box)` files.  None (default): no cut.  On a curvilinear file (2-D
    coordinates on the variable's last two dimensions) the box is the index rectangle of `curvilinear_box`, `cyclic` as
    there, under the same invariant.
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
        rec_shape = read_shape = r0.rec_shape
        cut, inner_read = None, 0
        if box is None and _check_cyclic(cyclic) != 'auto':
            raise ValueError('cyclic needs a box')
        if box is not None:                                       # records are read whole and cut on the device
            _grid_dims(r0.dims, var_name, ds0)
            cut = _Cut(ds0, None, box, r0.dims, cyclic)
            rec_shape = read_shape[:-2] + (cut.nlat_sel, cut.nlon_sel)
            inner_read = int(np.prod(read_shape, dtype=np.int64))
        inner = int(np.prod(rec_shape, dtype=np.int64))
        recs = _records_of_bins(bins, len(keys))
        ctx = default_context()
        nb = _fit_records(ctx, max(len(r) for r in recs), (inner + inner_read) * dt.itemsize, max_records)
        acc = _BinMean(ctx, rec_shape, dt, odt, nb)
        host = np.empty((nb,) + read_shape, dtype=dt)
        d_read = ctx.empty((nb,) + read_shape, dt) if cut is not None else None      # the uncut records of a chunk
        d_mean = ctx.empty(rec_shape, odt)
        result = np.empty((len(keys),) + rec_shape, dtype=odt)

        def fill(d_chunk, part):
            for i, r in enumerate(part):
                k, j = where[r]
                host[i] = opened[k][1].read_record(j)
            if cut is None:
                DeviceArray(ctx, (len(part),) + rec_shape, dt, ptr=d_chunk.ptr, owner=d_chunk).copy_from(host[:len(part)])
                return
            DeviceArray(ctx, (len(part),) + read_shape, dt, ptr=d_read.ptr, owner=d_read).copy_from(host[:len(part)])
            planes = len(part) * int(np.prod(read_shape[:-2], dtype=np.int64))
            _launch_select(ctx, dt.itemsize, planes, 1, read_shape[-2], read_shape[-1], d_read.ptr, None,
                           (cut.lat0, cut.nlat_sel), (cut.lon0, cut.nlon_sel), 1, 0, d_chunk.ptr)

        for k, part in enumerate(recs):
            acc.run(part, fill, d_mean)
            result[k] = d_mean.numpy()
        t_out = np.array([times[part[-1]] for part in recs], dtype=times.dtype)
    finally:
        for _, rd in opened:
            rd.close()
    result, vattrs = _encoded(result, ds0[var_name].attrs)
    out = ncio.Dataset(attrs=dict(ds0.attrs), record_dim=ds0.record_dim)
    coords = {d: ds0[d].values for d in r0.dims[1:] if d in ds0} if cut is None else {}
    coords[tdim] = t_out
    for name, f in ds0.variables.items():
        if name == var_name:
            out[name] = ncio.Field(result, r0.dims, coords, vattrs)
        elif name == tdim:
            out[name] = ncio.Field(t_out, (tdim,), {tdim: t_out}, {k: v for k, v in f.attrs.items() if k != 'bounds'})
        elif tdim not in f.dims:
            out[name] = ncio.Field(f.values, f.dims, f.coords, dict(f.attrs)) if cut is None else cut.field(name, f)
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


def _parse_floats(text, what, n=None):
    if text is None:
        return None
    try:
        vals = [float(t) for t in str(text).split(',')]
    except ValueError:
        raise ValueError('%s must be comma separated numbers, got %r' % (what, text)) from None
    if n is not None and len(vals) != n:
        raise ValueError('%s must be %d comma separated numbers, got %r' % (what, n, text))
    return vals


def _join_box_option(argv):
    """`-b -73,37,-42,34`: argparse takes a value that starts with a minus sign and is not a plain number for an option;
    the value is joined to its flag (`--box=-73,37,-42,34`), which argparse accepts."""
    out, argv = [], list(argv)
    while argv:
        a = argv.pop(0)
        if a in ('-b', '--box') and argv and argv[0][:1] == '-' and argv[0][1:2] in tuple('0123456789.'):
            a = '--box=' + argv.pop(0)
        out.append(a)
    return out


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
                                            'climatologies and climate deltas, level / lon-lat box selection and the '
                                            'model-top merge.')
    sub = p.add_subparsers(dest='command', required=True)
    box_help = 'LON1,LON2,LAT1,LAT2: cut to this longitude-latitude box (cdo sellonlatbox; may wrap across 0 deg)'
    cyclic_help = ('with a box on a curvilinear grid (2-D latitude / longitude): does the grid close on itself along its last '
                   'dimension - decided from the coordinates (auto), yes or no; with 1-D coordinates only auto is allowed')
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
    c.add_argument('-b', '--box', type=str, default=None, help=box_help + ' in front of the climatology')
    c.add_argument('--cyclic', type=str, default='auto', choices=list(CYCLIC_CHOICES), help=cyclic_help)
    d = sub.add_parser('delta', help='Scenario climatology minus historical climatology (cdo sub)')
    d.add_argument('scen_file', type=str, help='{} is replaced by the variable name (also in the other two paths)')
    d.add_argument('hist_file', type=str)
    d.add_argument('delta_file', type=str)
    d.add_argument('-v', '--var_names', type=str, required=True, help='comma separated variable names')
    s = sub.add_parser('select', help='Select pressure levels and / or a lon-lat box of a file (cdo sellevel, sellonlatbox)')
    s.add_argument('-i', '--input', type=str, required=True, help='NetCDF-3 input file; {} is replaced by the variable name')
    s.add_argument('-o', '--output', type=str, required=True, help='output file; {} is replaced by the variable name')
    s.add_argument('-v', '--var_names', type=str, required=True, help='comma separated variable names, e.g. ta,hur,ua,va')
    s.add_argument('-l', '--levels', type=str, default=None, help='comma separated level values to keep, e.g. 100000,85000,50000')
    s.add_argument('-b', '--box', type=str, default=None, help=box_help)
    s.add_argument('--cyclic', type=str, default='auto', choices=list(CYCLIC_CHOICES), help=cyclic_help)
    s.add_argument('--max_records', type=int, default=None, help='at most this many time records per launch')
    m = sub.add_parser('merge_levels', help='Levels of FILE_A, then levels of FILE_B, as one variable (cdo sellevel, sellevel, '
                                            'merge: Emon_add_top_from_Amon.sh)')
    m.add_argument('file_a', type=str, help='{} is replaced by the variable name (also in the other two paths)')
    m.add_argument('file_b', type=str)
    m.add_argument('out_file', type=str)
    m.add_argument('-v', '--var_names', type=str, required=True, help='comma separated variable names, e.g. ua,va,ta,zg,hur')
    m.add_argument('--levels_a', type=str, default=None, help='comma separated level values to take from FILE_A (default: all)')
    m.add_argument('--levels_b', type=str, default=None, help='comma separated level values to take from FILE_B (default: all)')
    m.add_argument('--max_records', type=int, default=None, help='at most this many time records per launch')
    return p


def main(argv=None):
    args = build_parser().parse_args(_join_box_option(sys.argv[1:] if argv is None else argv))
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
                                          args.mode, years=years, max_records=args.max_records, out_dtype=args.out_dtype,
                                          box=_parse_floats(args.box, 'box', 4), cyclic=args.cyclic))
    elif args.command == 'delta':
        names = args.var_names.split(',')
        paths = (args.scen_file, args.hist_file, args.delta_file)
        if len(names) > 1 and not all('{}' in p for p in paths):
            raise ValueError('several variables need {} in all three paths')
        for name in names:
            done.append(delta_files(*[p.replace('{}', name) for p in paths], name))
    elif args.command == 'select':
        names = args.var_names.split(',')
        if len(names) > 1 and ('{}' not in args.input or '{}' not in args.output):
            raise ValueError('several variables need {} in the input and the output path')
        levels, box = _parse_floats(args.levels, 'levels'), _parse_floats(args.box, 'box', 4)
        if levels is None and box is None:
            raise ValueError('select needs --levels and / or --box')
        for name in names:
            done.append(select_file(args.input.replace('{}', name), args.output.replace('{}', name), name, levels=levels, box=box,
                                    max_records=args.max_records, cyclic=args.cyclic))
    elif args.command == 'merge_levels':
        names = args.var_names.split(',')
        paths = (args.file_a, args.file_b, args.out_file)
        if len(names) > 1 and not all('{}' in p for p in paths):
            raise ValueError('several variables need {} in all three paths')
        for name in names:
            done.append(merge_levels_files(*[p.replace('{}', name) for p in paths], name,
                                           levels_a=_parse_floats(args.levels_a, 'levels_a'),
                                           levels_b=_parse_floats(args.levels_b, 'levels_b'), max_records=args.max_records))
    else:
        raise ValueError('unknown command %r' % (args.command,))
    return done


if __name__ == '__main__':
    main()
