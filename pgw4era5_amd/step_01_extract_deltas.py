"""
step_01: the two array programs of the reference's step_01_extract_deltas directory on MI355X.

* `CFday_interp_to_plev.py:86-154`: daily CMIP6 `CFday` fields on the GCM's hybrid model levels (`ap`, `b`, `ps` in the
  file) interpolated to a fixed list of pressure levels -> `interp_to_plev` / `interp_file` / sub-command `interp_to_plev`.
  One fused kernel (`pgw_interp_hybrid_to_plev`): the source pressure `ap + b * ps` is formed per column in registers and
  the logarithms of the target list are taken once per thread block; neither 4-D pressure field of the reference
  (`source_P`, `targ_P`, :91 and :115-122) exists on the host or on the device.
* `Emon_convert_hus_to_hur.py:16-21, 45-123`: monthly `Emon` specific humidity -> relative humidity with the script's own
  Magnus formula (`specific_to_relative_humidity` HERE is that one; `functions.specific_to_relative_humidity` is the IFS
  formula of the reference's functions.py), then the coarse `Amon` hur carried onto the finer `Emon` levels with weights
  taken from the computed hur (`merge_hur_levels`) -> `hus_to_hur_file` / sub-command `hus_to_hur`.

The shell templates of step_01 (`cdo`, `wget`) are site scripts and stay out of scope.

Array kinds as in `functions.py`: numpy, `ncio.Field` (labels re-wrapped) or `DeviceArray` in, the same kind out.
Files are NetCDF-3 through `ncio` like everywhere in this package.
"""
import argparse
import ctypes as C
import os

import numpy as np

from . import _lib, ncio
from .device import DeviceArray, default_context, dtype_tag
from .functions import _check_extrapolate, _dev, _is_labelled, _raw
from .settings import LAT_GCM, LEV_GCM, LON_GCM, PLEV_GCM, TIME_GCM

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_F32, _F64 = np.dtype('float32'), np.dtype('float64')

MAX_LEVELS = 256          # nsrc, ntarg, nplev limit of the kernels (include/pgw_hip.h)


def _f64(x, name):
    a = np.ascontiguousarray(_raw(x), dtype=np.float64)
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
    dt = _F32 if (np.dtype(var_dtype) == _F32 and np.dtype(ps_dtype) == _F32) else _F64
    odt = _F64 if out_dtype is None else np.dtype(out_dtype)
    if odt not in (_F32, _F64) or (odt == _F32 and dt != _F32):
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
    mode = _check_extrapolate(extrapolate)
    rv, rp = _raw(var), _raw(ps)
    if len(rv.shape) != 4:
        raise ValueError('expected a 4-D (time, lev, lat, lon) array, got shape %s' % (rv.shape,))
    nt, S, nlat, nlon = rv.shape
    if tuple(rp.shape) != (nt, nlat, nlon):
        raise ValueError('ps must be (time, lat, lon) = %s, got %s' % ((nt, nlat, nlon), tuple(rp.shape)))
    ap, b, targ, dt, odt = _hybrid_args(rv.dtype, rp.dtype, S, ap, b, targ_plev, out_dtype)
    src_rev = levels_descend(ap, b) if lev_descending is None else bool(lev_descending)
    ctx = default_context()
    d_var, d_ps = _dev(ctx, var, dt), _dev(ctx, ps, dt)
    out = ctx.empty((nt, len(targ), nlat, nlon), odt)
    _launch_hybrid(ctx, d_var, d_ps, ap, b, targ, mode, src_rev, plev_descending, out)
    if isinstance(rv, DeviceArray):
        return out
    host = out.numpy()
    if _is_labelled(var):
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
    per = (S * s_in + s_in + N * s_out) * ncol
    free, _ = ctx.mem_info()
    n = max(1, min(int(nrec), int(0.8 * free) // max(per, 1)))
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
    mode = _check_extrapolate(extrapolate)
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
    rq, rt = _raw(QV), _raw(T)
    if tuple(rq.shape) != tuple(rt.shape) or len(rq.shape) != 4:
        raise ValueError('QV and T must be 4-D (time, plev, lat, lon) arrays of one shape')
    nt, nplev, nlat, nlon = rq.shape
    p = np.asarray(_raw(P), dtype=np.float64) if not isinstance(_raw(P), DeviceArray) else _raw(P).numpy().astype(np.float64)
    if p.ndim == 4:
        if p.shape != tuple(rq.shape) or not np.array_equal(p, np.broadcast_to(p[0, :, 0, 0][None, :, None, None], p.shape), equal_nan=True):
            raise ValueError('a 4-D P must hold the same pressure list in every column')
        p = p[0, :, 0, 0]
    p = np.ascontiguousarray(p.reshape(-1))
    if len(p) != nplev or nplev > MAX_LEVELS:
        raise ValueError('P must hold the %d pressure levels of QV (at most %d)' % (nplev, MAX_LEVELS))
    dt = _F32 if (rq.dtype == _F32 and rt.dtype == _F32) else _F64
    ctx = default_context()
    d_q, d_t = _dev(ctx, QV, dt), _dev(ctx, T, dt)
    out = ctx.empty(rq.shape, _F64)
    ctx._check(ctx.lib.pgw_magnus_rh(ctx.handle, dtype_tag(dt), nt, nplev, nlat * nlon, d_q.ptr, _cdp(p), d_t.ptr, out.ptr))
    if isinstance(rq, DeviceArray):
        return out
    host = out.numpy()
    return QV.like(host) if (_is_labelled(QV) and hasattr(QV, 'like')) else host


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
    if _is_labelled(hur) and _is_labelled(amon_hur):
        _same_coords(hur, amon_hur, 'merge_hur_levels')
    rh, ra = _raw(hur), _raw(amon_hur)
    if len(rh.shape) != 4 or len(ra.shape) != 4:
        raise ValueError('hur and amon_hur must be 4-D (time, plev, lat, lon)')
    nt, nplev, nlat, nlon = rh.shape
    if (ra.shape[0], ra.shape[2], ra.shape[3]) != (nt, nlat, nlon):
        raise ValueError('hur %s and amon_hur %s differ in time / lat / lon' % (tuple(rh.shape), tuple(ra.shape)))
    tabs = merge_level_table(plev, amon_plev)
    if len(tabs[0]) != nplev or len(_f64(amon_plev, 'amon_plev')) != ra.shape[1] or nplev > MAX_LEVELS:
        raise ValueError('plev / amon_plev do not match the level axes of the fields')
    adt = _F32 if ra.dtype == _F32 else _F64
    ctx = default_context()
    d_h, d_a = _dev(ctx, hur, _F64), _dev(ctx, amon_hur, adt)
    out = ctx.empty(rh.shape, _F64)
    ti = [np.ascontiguousarray(t, dtype=np.int32) for t in tabs]
    ctx._check(ctx.lib.pgw_hur_merge_levels(ctx.handle, dtype_tag(adt), nt, nplev, ra.shape[1], nlat * nlon, d_h.ptr, d_a.ptr,
                                            *[t.ctypes.data_as(_ip) for t in ti], out.ptr))
    if isinstance(rh, DeviceArray):
        return out
    host = out.numpy()
    return hur.like(host) if (_is_labelled(hur) and hasattr(hur, 'like')) else host


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


# ------------------------------------------------------------------------------- command line
def build_parser():
    p = argparse.ArgumentParser(prog='python -m pgw4era5_amd.step_01_extract_deltas',
                                description='PGW for ERA5 step_01 on MI355X: CFday model levels to pressure levels, Emon hus to hur.')
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
    else:
        done.append(hus_to_hur_file(args.hus_file, args.ta_file, args.hur_file, args.amon_hur_file))
    return done


if __name__ == '__main__':
    main()
