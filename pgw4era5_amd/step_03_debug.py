"""
step_03 `--debug_mode`: the climate deltas written out instead of the ERA5 files (reference
step_03_apply_to_era.py:350-361 `interpolate_full`, :387-414 `interpolate_time`).

A validation aid: with real ERA5 and GCM files a user compares the delta this port adds with the delta the reference adds,
variable by variable (tools/compare_deltas.py) - an ERA5 state hides a 1e-3 K disagreement under 300 K.

Both functions are synchronous per file - read, upload, compute, download, write - and stand beside the pipelined driver:
no device buffer sets, no pinned pools, no `stages` attribute (parallel.run_shard therefore calls them file by file).

`interpolate_full` runs the normal per-file computation (process_file_device, every mode it has) and then asks the GPU for
the deltas themselves: `pgw_delta_fields` (the values k_delta_quad adds, with its expressions: era + delta reproduces the
outputs bit for bit), `pgw_surface_deltas`, and ps_pgw - PS (`pgw_field_sub`).  Files are NetCDF-3 (ncio.to_netcdf); the
attributes xarray would write cannot be pinned here: variable, dims, coordinate variables and the
source variable's attributes are written.
"""
import os

import numpy as np

from . import _lib
from . import settings as S
from ._lib import _dp
from .device import default_context, dtype_tag

FULL_VARS = ('ps', 'ta', 'hur', 'ua', 'va', 'st', 'ts')                          # step_03:351
TIME_VARS = ('tos', 'tas', 'hurs', 'ps', 'ta', 'hur', 'ua', 'va', 'zg')          # step_03:401


def full_delta_path(out_era_file_path, var_name):
    """`{var_name_map[var]}_delta_{name of the output file}` beside the output file (step_03:355-357)."""
    return os.path.join(os.path.dirname(out_era_file_path),
                        '{}_delta_{}'.format(S.var_name_map[var_name], os.path.basename(out_era_file_path)))


def time_delta_path(out_era_file_path, var_name):
    """`delta_{var}_{name of the output file}` beside the output file (step_03:405-407)."""
    return os.path.join(os.path.dirname(out_era_file_path),
                        '{}_{}_{}'.format('delta', var_name, os.path.basename(out_era_file_path)))


def _coord_fields(ds, src, dims, time_field=None):
    """Coordinate variables of `dims` into the Dataset `ds`, taken from the dataset `src` (values and attributes);
    the time axis is replaced by `time_field` when given (functions.py:296)."""
    from . import ncio
    for d in dims:
        if time_field is not None and d == time_field.dims[0]:
            ds[d] = ncio.Field(time_field.values, (d,), {}, time_field.attrs)
        elif d in src and src[d].dims == (d,):
            ds[d] = ncio.Field(src[d].values, (d,), {}, src[d].attrs)


def _write(path, name, values, dims, src, attrs, time_field=None):
    from . import ncio
    ds = ncio.Dataset()
    _coord_fields(ds, src, dims, time_field)
    ds[name] = ncio.Field(values, dims, {d: ds[d].values for d in dims if d in ds}, attrs)
    ncio.to_netcdf(ds, path)


# ----------------------------------------------------------------------------------------
# interpolate_time                                                       step_03:387-414
# ----------------------------------------------------------------------------------------
def time_interpolated_delta(ctx, values, delta_times, target_dt):
    """load_delta's time interpolation (functions.py:224-292) of an in-memory record array on the GPU: the record itself in
    the file's dtype when the instant is one (:282-283), else float64 (`pgw_time_lerp_mixed`: y_hi - y_lo in the records'
    dtype, slope and result float64; float64 records: `pgw_time_lerp`).  Returns (1,) + record shape."""
    from .step_03_apply_to_era import delta_time_bracket
    ib, ia, x_hi, x_new, keep = delta_time_bracket(delta_times, target_dt)
    vb = np.asarray(values[keep[ib]])
    if x_hi == 0.0:
        return np.array(vb, copy=True)[None]
    dt = vb.dtype if vb.dtype in (np.dtype('float32'), np.dtype('float64')) else np.dtype('float64')
    b = ctx.to_device(np.ascontiguousarray(vb, dtype=dt), dt)
    a = ctx.to_device(np.ascontiguousarray(values[keep[ia]], dtype=dt), dt)
    out = ctx.empty((1,) + b.shape, np.float64)
    if dt == np.dtype('float64'):
        ctx._check(ctx.lib.pgw_time_lerp(ctx.handle, _lib.PGW_F64, b.size, b.ptr, a.ptr, x_hi, x_new, out.ptr))
    else:
        ctx._check(ctx.lib.pgw_time_lerp_mixed(ctx.handle, dtype_tag(dt), dtype_tag(dt), b.size, b.ptr, a.ptr, x_hi, x_new,
                                               out.ptr))
    return out.numpy()


def debug_interpolate_time(inp_era_file_path, out_era_file_path, delta_input_dir, era_step_dt,
                           ignore_top_pressure_error, debug_mode=None):
    """`--debug_mode interpolate_time` (step_03:387-414): every delta interpolated in time only, written as
    `delta_{var}_{name}` beside the output path; `ps` is ps_delta.nc.  The ERA5 file is opened for its time axis alone."""
    from . import ncio
    ctx = default_context()
    if S.i_debug >= 0:
        print('Start working on input file {}'.format(inp_era_file_path))
    era_time = ncio.RecordReader(inp_era_file_path, S.TIME_ERA, decode_times=False)          # header and time axis only
    time_field = ncio.Field(np.asarray(era_time.coords[S.TIME_ERA]).reshape(-1)[:1], (S.TIME_GCM,), {}, era_time.attrs)
    era_time.close()
    from . import step_03_apply_to_era as s3
    era5, pole, winds = None, None, {}
    mode = s3.delta_grid_mode()
    if mode != 'era5':                                      # the deltas lie on the GCM's grid: regridded here, by step_02's calls
        from .functions import interp_wrapper, regrid_lat_lon_wind
        era5 = s3._open_era5_target(inp_era_file_path)
        if mode == 'source':
            s3._mesh_axes(era5)
        else:
            pole = s3._rotation_pole(era5, s3.era_layout(era5))
    for var in TIME_VARS:
        ds = ncio.open_dataset(os.path.join(delta_input_dir, S.file_name_bases['SCEN-HIST'].format(var)))      # functions.py:203
        if pole is not None and var in ('ua', 'va'):        # rotated together, as step_02 regridding --rotate_winds writes them
            if not winds:
                other = 'va' if var == 'ua' else 'ua'
                pair = {var: ds, other: ncio.open_dataset(os.path.join(delta_input_dir, S.file_name_bases['SCEN-HIST'].format(other)))}
                winds = dict(zip(('ua', 'va'), regrid_lat_lon_wind(pair['ua'], pair['va'], era5, pole)))
            ds = winds[var]
        elif era5 is not None:
            ds = interp_wrapper(ds, era5, var, i_use_xesmf=0, nan_interp_kernel_radius=S.nan_interp_kernel_radius,
                                nan_interp_sharpness=S.nan_interp_sharpness)
        fld = ds[var]
        if fld.dims[0] != S.TIME_GCM or S.TIME_GCM not in ds:
            raise ValueError('first dimension of %s must be %s with a coordinate variable' % (var, S.TIME_GCM))
        val = time_interpolated_delta(ctx, fld.values, np.asarray(ds[S.TIME_GCM].values), era_step_dt)
        _write(time_delta_path(out_era_file_path, var), var, val, fld.dims, ds, fld.attrs, time_field)
    return None


# ----------------------------------------------------------------------------------------
# interpolate_full                                                       step_03:350-361
# ----------------------------------------------------------------------------------------
def delta_fields_device(ctx, ps, deltas, target_dt, nlev, ref, ignore_top_pressure_error=False, scratch=None):
    """The four deltas of load_delta_interp on the model levels of the surface pressure `ps` (a DeviceArray (1, nlat, nlon) in
    the deltas' dtype; levels of the context's last set_levels): one `pgw_delta_fields` call on the records
    process_file_device hands to pgw_step03_file.  Returns dict ta, hur, ua, va of float64 DeviceArrays (1, nlev, nlat, nlon)."""
    scratch = {} if scratch is None else scratch

    def buf(name, shape, dtype=deltas.dtype):
        if name not in scratch or scratch[name].shape != tuple(shape) or scratch[name].dtype != np.dtype(dtype):
            scratch[name] = ctx.empty(shape, dtype)
        return scratch[name]

    _lib.check_nplev(len(deltas.plev))
    _, _, x_hi, x_new, _ = deltas.bracket(target_dt, 'ta')
    rec = []
    for var in ('ta', 'hur', 'ua', 'va', 'tas', 'hurs', 'ps_hist'):
        rec += list(deltas.pair_on_axis_of(var, target_dt, (x_hi, x_new), buf))
    nt, nlat, nlon = ps.shape
    out = {k: buf('_d' + k, (nt, nlev, nlat, nlon), np.float64) for k in ('ta', 'hur', 'ua', 'va')}
    plev = deltas.plev
    ctx._check(ctx.lib.pgw_delta_fields(ctx.handle, dtype_tag(deltas.dtype), 1 if ref else 0, nt, nlev, len(plev), nlat * nlon,
                                        plev.ctypes.data_as(_dp), ps.ptr, *[r.ptr for r in rec], x_hi, x_new,
                                        1 if ignore_top_pressure_error else 0, *[out[k].ptr for k in ('ta', 'hur', 'ua', 'va')]))
    return out


def surface_deltas_device(ctx, era, coeffs, deltas, target_dt, ref, scratch=None):
    """delta_ts_combined (step_03:118-125) and delta_soilt (:139-143) of one file: `pgw_surface_deltas` on the record pairs
    and time axes process_file_device hands to pgw_step03_file.  Returns float64 DeviceArrays (ts (1, nlat, nlon), st (1, nsoil, nlat, nlon))."""
    scratch = {} if scratch is None else scratch
    soil = np.ascontiguousarray(coeffs['soil1'], dtype=np.float64)
    nt, nlat, nlon = era['FR_SEA_ICE'].shape
    args = []
    for var in ('siconc', 'tos', 'ts'):
        b_, a_, vx_hi, vx_new = deltas.pair(var, target_dt, None)
        args += [b_.ptr, a_.ptr, vx_hi, vx_new]
    ts = scratch['_dts'] = ctx.empty((nt, nlat, nlon), np.float64)
    st = scratch['_dst'] = ctx.empty((nt, len(soil), nlat, nlon), np.float64)
    ctx._check(ctx.lib.pgw_surface_deltas(ctx.handle, dtype_tag(deltas.dtype), 1 if ref else 0, nt, nlat * nlon, len(soil),
                                          soil.ctypes.data_as(_dp), era['FR_SEA_ICE'].ptr, *args, era['FR_LAND'].ptr,
                                          deltas.ts_clim.ptr, ts.ptr, st.ptr))
    return ts, st


def debug_interpolate_full(inp_era_file_path, out_era_file_path, delta_input_dir, era_step_dt,
                           ignore_top_pressure_error, debug_mode='interpolate_full'):
    """`--debug_mode interpolate_full` (step_03:350-361) for one file: the normal computation, then the seven deltas ps, ta,
    hur, ua, va, st, ts as `{var_name_map[v]}_delta_{name}` beside the output path; no ERA5 file is written.  ta / hur (and
    ua / va) stand on the levels of the file's PS, under settings.i_reinterp = 1 on those of the converged ps_pgw
    (:212-216, 336-343).  Returns the number of loop passes."""
    from . import ncio
    from . import step_03_apply_to_era as s3
    ctx = default_context()
    if S.i_debug >= 0:
        print('Start working on input file {}'.format(inp_era_file_path))
    era_file = ncio.open_dataset(inp_era_file_path, decode_times=False)                          # step_03:60
    vm = S.var_name_map
    dtype = np.dtype('float64') if era_file[vm['ta']].dtype.itemsize == 8 else np.dtype('float32')
    H = s3.era_layout(era_file)                             # (lat, lon), or the dimensions of 2-D lat / lon, or (cell,)
    dims = s3.layout_dims(H)
    dims3, dims4, dims_so = dims['d3'], dims['d4'], dims['so']
    if not s3.is_mesh(H):
        for key, d in s3._FIELD_DIMS.items():
            s3._check_dims(vm[key], era_file[vm[key]], dims[d], inp_era_file_path)

    def get(name, dims):
        return s3._as_grid(np.ascontiguousarray(era_file[name].transpose(*dims).values, dtype=dtype), H)

    era = dict(PS=get(vm['ps'], dims3), FIS=get(vm['zgs'], dims3), T=get(vm['ta'], dims4), QV=get(vm['hus'], dims4),
               U=get(vm['ua'], dims4), V=get(vm['va'], dims4), T_SKIN=get(vm['ts'], dims3),
               T_SO=get(vm['st'], dims_so), FR_LAND=get(vm['sftlf'], dims3), FR_SEA_ICE=get(vm['sic'], dims3))
    coeffs = dict(ak=np.asarray(era_file['ak'].values, dtype=np.float64), bk=np.asarray(era_file['bk'].values, dtype=np.float64),
                  soil1=np.asarray(era_file[S.SOIL_HLEV_ERA].values, dtype=np.float64))
    if 'akm' in era_file:                                                                        # step_03:68-70
        coeffs['akm'] = np.asarray(era_file['akm'].values, dtype=np.float64)
        coeffs['bkm'] = np.asarray(era_file['bkm'].values, dtype=np.float64)
    deltas = s3.load_delta_set(ctx, delta_input_dir, dtype, era5=(era_file, inp_era_file_path))
    e = s3._upload_era(ctx, era, dtype)
    ref = s3.ref_dtype_mode(dtype)
    try:
        out, info = s3.process_file_device(ctx, e, coeffs, deltas, era_step_dt, ignore_top_pressure_error,
                                           p_ref='local' if S.p_ref_inp is None else S.p_ref_inp,
                                           i_reinterp=bool(S.i_reinterp))
    except ValueError as err:
        if getattr(err, 'status', None) == _lib.PGW_ERR_NOT_CONVERGED:                           # step_03:315-319
            raise ValueError('ERROR! Pressure adjustment did not converge for file {}. Consider increasing the value for '
                             '"max_n_iter" in settings.py'.format(inp_era_file_path)) from None
        raise
    scratch = {}
    ps_levels = out['PS'] if S.i_reinterp else e['PS']
    d4 = delta_fields_device(ctx, ps_levels, deltas, era_step_dt, era['T'].shape[1], ref, ignore_top_pressure_error, scratch)
    d_ts, d_st = surface_deltas_device(ctx, e, coeffs, deltas, era_step_dt, ref, scratch)
    d_ps = ctx.empty(e['PS'].shape, dtype)                                                       # ps_pgw - PS, :326
    ctx._check(ctx.lib.pgw_field_sub(ctx.handle, dtype_tag(dtype), d_ps.size, out['PS'].ptr, e['PS'].ptr, d_ps.ptr))
    results = dict(ps=(d_ps, dims3), ta=(d4['ta'], dims4), hur=(d4['hur'], dims4), ua=(d4['ua'], dims4), va=(d4['va'], dims4),
                   st=(d_st, dims_so), ts=(d_ts, dims3))
    for var in FULL_VARS:
        arr, dims = results[var]
        name = vm[var]
        attrs = era_file[name].attrs if name in era_file else {}
        _write(full_delta_path(out_era_file_path, var), name, s3._as_file(arr.numpy(), H), dims, era_file, attrs)
    if S.i_debug >= 2:
        for it, err in enumerate(info['max_err']):
            print('### iteration {:03d}, phi max error: {}'.format(it + 1, err))
    return info['n_iter']
