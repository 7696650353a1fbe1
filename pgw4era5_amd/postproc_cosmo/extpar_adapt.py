"""
COSMO-specific: perturb the deep soil temperature climatology T_CL of an extpar file with the ts climate delta on MI355X.

Program and command line of the reference's postproc_cosmo/extpar_adapt.py (:13-63): positional extpar_file_path,
-d/--delta_input_dir.  The delta directory holds `ts_delta.nc` on the grid of the extpar file, e.g. from
`step_02_preproc_deltas regridding -e EXTPAR -v ts` under default settings (an extpar file on a rotated grid has 2-D lat /
lon: a regular-grid delta is interpolated onto them point by point, functions.regrid_points).

    delta_ts      = load_delta(delta_inp_path, 'ts', None)           # every record                       :20
    delta_ts_clim = delta_ts.mean(dim=['time'])                      # np.nanmean over the records        :29
    ext_file['T_CL'][:] += delta_ts_clim.values.squeeze()            # in place, masked cells kept        :32

The mean and the addition are one kernel (`pgw_time_mean_add`, include/pgw_hip.h); T_CL travels as the file's raw words,
its byte order is converted on the device both ways, and `ncio.update_variable` writes the variable's bytes back into the
file - no other byte of it changes.  Like the reference, a second run adds the delta a second time.
"""
import argparse

import numpy as np

from .. import ncio
from ..device import DeviceArray, default_context
from ..functions import load_delta, time_mean_add

var_name_map = {
    'ts':   'T_CL',
}

NC_FILL = 9.969209968386869e36          # NC_FILL_FLOAT = NC_FILL_DOUBLE: what netCDF4 masks when a variable names no fill value


def mask_values(attrs):
    """The values netCDF4-python's automatic masking hides from the in-place addition: `_FillValue` and `missing_value` of
    the variable (either, both), or NetCDF's default fill value when it has neither.  valid_min / valid_max / valid_range
    are not looked at."""
    vals = []
    for key in ('_FillValue', 'missing_value'):
        if key in attrs:
            vals += [float(a) for a in np.atleast_1d(np.asarray(attrs[key]))]
    if len(vals) > 2:
        raise ValueError('%s: more than two fill / missing values (%s) are not supported' % (var_name_map['ts'], vals))
    return vals if vals else [NC_FILL]


def _read_t_cl(ext_file_path):
    """T_CL as the file holds it (big-endian words) with its mask values; ValueError for a file this program cannot adapt."""
    name = var_name_map['ts']
    try:
        raw, dims, attrs = ncio.read_variable_raw(ext_file_path, name)
    except KeyError:
        raise ValueError('%s has no variable %s' % (ext_file_path, name)) from None
    if 'scale_factor' in attrs or 'add_offset' in attrs or raw.dtype.kind != 'f':
        raise ValueError('%s is stored packed (%s with scale_factor / add_offset); only float32 / float64 %s is supported'
                         % (name, raw.dtype, name))
    return raw, mask_values(attrs)


def extpar_adapt(ext_file_path, delta_inp_path):
    if delta_inp_path is None:
        raise ValueError('Delta input directory (-d) is required.')
    t_cl, masks = _read_t_cl(ext_file_path)

    # update T_CL
    print('update deep soil temperature')

    delta_ts = load_delta(delta_inp_path, 'ts', None)
    shp = tuple(delta_ts.shape[1:])
    lead = t_cl.ndim - len(shp)
    if lead < 0 or tuple(t_cl.shape[lead:]) != shp or any(k != 1 for k in t_cl.shape[:lead]):
        raise ValueError('%s %s and the ts delta %s are not on the same grid' % (var_name_map['ts'], tuple(t_cl.shape), shp))

    ctx = default_context()
    d_t = DeviceArray(ctx, t_cl.shape, t_cl.dtype.newbyteorder('=')).copy_from(t_cl)      # byte order converted on the device
    _, info = time_mean_add(d_t, delta_ts, masks, counts=True, out=d_t)                    # the one launch, in place
    mean, n_new_nan = info['mean'].numpy(), info['n_new_nan']
    with np.errstate(all='ignore'):
        print('delta_ts_clim: shape %s, min %s, max %s' % (mean.shape, np.nanmin(mean) if np.isfinite(mean).any() else np.nan,
                                                           np.nanmax(mean) if np.isfinite(mean).any() else np.nan))
    if n_new_nan > 0:
        print('WARNING: %d cells of %s became NaN (the ts delta is missing there in every record).' % (n_new_nan, var_name_map['ts']))
    host = np.empty(d_t.nbytes, dtype=np.uint8)
    new = d_t.download_foreign(host)                                                        # ... and back into the file's
    ctx.sync()
    ncio.update_variable(ext_file_path, var_name_map['ts'], new)
    print('Done.')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(
        prog='python -m pgw4era5_amd.postproc_cosmo.extpar_adapt',
        description='COSMO-specific: Perturb Extpar soil temperature climatology T_CL with the ts climate delta (on MI355X).')
    # extpar file to modify
    parser.add_argument('extpar_file_path', type=str, help='Path to extpar file to modify T_CL.')
    # climate delta directory (already remapped to the grid of the extpar file)
    parser.add_argument('-d', '--delta_input_dir', type=str, default=None,
                        help='Directory with GCM climate deltas to be used. This directory should have a climate delta for ts '
                             'already horizontally remapped to the grid of the extpar file, which can be done with '
                             'step_02_preproc_deltas.py (regridding -e EXTPAR -v ts, settings.i_use_xesmf_regridding = 1) '
                             'or otherwise with CDO.')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    print(args)
    extpar_adapt(args.extpar_file_path, args.delta_input_dir)


if __name__ == '__main__':
    main()
