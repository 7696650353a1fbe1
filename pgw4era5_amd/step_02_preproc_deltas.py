"""
step_02: regrid GCM climate deltas (and HIST climatologies) to the ERA5 grid on MI355X.

Command line of the reference's step_02_preproc_deltas.py (:27-87): positional
{smoothing,regridding}, -i, -o, -e, -v.  For every variable both `{var}_historical.nc` and
`{var}_delta.nc` are processed (:116-119).  `regridding` runs the bilinear lat-then-lon kernel
(functions.regrid_lat_lon; onto a target file with 2-D lat / lon over shared dimensions, such as an extpar file, its
point-wise form), or with settings.i_use_xesmf_regridding = 1 the cell-locate / sparse-apply kernels for source
grids with 2-D coordinates; `smoothing` runs the annual-cycle filter for daily deltas
(functions.filter_data, reference functions.py:603-740); tos / siconc on the ocean grid go through the
NaN-ignoring Gaussian-kernel interpolation (functions.nan_ignoring_interp, reference functions.py:900-1060), onto a
mesh or onto a target file with 2-D lat / lon alike.

Not in the reference: `--rotate_winds [auto | POLE_LAT,POLE_LON]` for a target file on a rotated-pole grid, whose U / V are
GRID-RELATIVE (U along increasing rlon, V along increasing rlat) while the GCM's ua / va are eastward / northward: ua and
va of each period are regridded together and rotated onto the grid's directions (functions.regrid_lat_lon_wind), so that
step_03 adds like to like.  Off by default; with it off nothing about a run differs.
"""
import argparse
import os
from pathlib import Path

from . import ncio
from .functions import filter_data, interp_wrapper, regrid_lat_lon_wind, check_wind_pair, rotated_pole_of, _Target
from . import settings
from .settings import file_name_bases, nan_interp_kernel_radius, nan_interp_sharpness, LAT_ERA, LON_ERA

DEFAULT_VARS = 'ta,hur,ua,va,zg,hurs,tas,ps,tos,ts,siconc'
WINDS = ('ua', 'va')
PERIODS = ('HIST', 'SCEN-HIST')


def parser():
    p = argparse.ArgumentParser(description='PGW for ERA5: regrid GCM deltas to the ERA5 grid (MI355X).')
    p.add_argument('processing_step', type=str, choices=['smoothing', 'regridding'])
    p.add_argument('-i', '--input_dir', type=str, help='directory with {var}_delta.nc and {var}_historical.nc')
    p.add_argument('-o', '--output_dir', type=str, help='directory for the regridded files')
    p.add_argument('-e', '--era5_file_path', type=str, default=None, help='example ERA5 file (target grid)')
    p.add_argument('-v', '--var_names', type=str, default=DEFAULT_VARS, help='comma separated variable names')
    p.add_argument('--rotate_winds', type=str, nargs='?', const='auto', default=None, metavar='auto|POLE_LAT,POLE_LON',
                   help='regridding onto a rotated-pole target file: write ua / va as grid-relative components (along rlon / '
                        'rlat) instead of eastward / northward.  auto (the value when none is given): the pole is taken from '
                        "the target file's rotated_latitude_longitude mapping; or the geographic position of the grid's north "
                        'pole in degrees.  Default: off')
    return p


def wind_pole(rotate_winds, ds_era5):
    """The value of `--rotate_winds` -> (pole_lat, pole_lon): `auto` from the rotated mapping of the target file (rotated_pole_of),
    else POLE_LAT,POLE_LON parsed and checked.  ValueError naming the cause.  Also the rule of step_03's --rotate_winds."""
    if rotate_winds == 'auto':
        return rotated_pole_of(ds_era5, settings.var_name_map['ua'])
    try:
        lat, lon = (float(x) for x in rotate_winds.split(','))
    except ValueError:
        raise ValueError("--rotate_winds takes 'auto' or POLE_LAT,POLE_LON in degrees, got %r" % rotate_winds) from None
    if not (-90.0 <= lat <= 90.0 and -360.0 <= lon <= 360.0):
        raise ValueError('--rotate_winds: a pole at latitude %r, longitude %r is not a position in degrees' % (lat, lon))
    return (lat, lon)


def _wind_plan(args, var_names, ds_era5):
    """Everything `--rotate_winds` can object to, before a file is written -> (pole, {period: (ds_ua, ds_va)}), the input
    files opened.  ValueError naming the cause."""
    if args.processing_step == 'smoothing':
        raise ValueError('--rotate_winds belongs to the regridding step: smoothing runs on the GCM grid, where the winds are '
                         'geographic')
    if settings.i_use_xesmf_regridding:
        raise ValueError('--rotate_winds with settings.i_use_xesmf_regridding = 1 is not built: a curvilinear or rotated source '
                         'grid may carry grid-relative winds of its own, which would have to be turned to geographic first')
    if not _Target.of(ds_era5[LAT_ERA], ds_era5[LON_ERA]).points:
        raise ValueError('--rotate_winds: the target file has 1-D lat / lon axes - the winds of a lat-lon mesh are geographic '
                         'already, there is nothing to rotate')
    have = [w in var_names for w in WINDS]
    if have[0] != have[1]:
        raise ValueError('--rotate_winds needs ua and va together: -v lists %s without %s'
                         % ((WINDS[0], WINDS[1]) if have[0] else (WINDS[1], WINDS[0])))
    pole = wind_pole(args.rotate_winds, ds_era5)
    pairs = {}
    if have[0]:
        for period in PERIODS:
            paths = [os.path.join(args.input_dir, file_name_bases[period].format(w)) for w in WINDS]
            for w, path in zip(WINDS, paths):
                if not os.path.exists(path):
                    raise ValueError('Files for variable ' + w + ' are missing')
            pairs[period] = tuple(ncio.open_dataset(path) for path in paths)
            check_wind_pair(*pairs[period], names=WINDS)
    return pole, pairs


def main(argv=None):
    args = parser().parse_args(argv)
    print(args)
    if args.input_dir is None:
        raise ValueError('Input directory (-i) is required.')
    if args.output_dir is None:
        raise ValueError('Output directory (-o) is required.')
    if args.processing_step == 'regridding' and args.era5_file_path is None:
        raise ValueError('era5_file_path is required for regridding step.')
    Path(args.output_dir).mkdir(exist_ok=True, parents=True)
    var_names = args.var_names.split(',')
    print('Run {} for variable names {}.'.format(args.processing_step, var_names))
    smoothing = args.processing_step == 'smoothing'
    ds_era5 = None if smoothing else ncio.open_dataset(args.era5_file_path, decode_times=False)
    pole, wind_pairs = _wind_plan(args, var_names, ds_era5) if args.rotate_winds is not None else (None, {})
    rotated = {}                                             # period -> {'ua': dataset, 'va': dataset}, made when the first is due
    done = []
    for var_name in var_names:
        print(var_name)
        if smoothing:                                        # step_02_preproc_deltas.py:129-132
            for clim_period in PERIODS:
                fname = file_name_bases[clim_period].format(var_name)
                inp, out = os.path.join(args.input_dir, fname), os.path.join(args.output_dir, fname)
                filter_data(inp, var_name, out)
                done.append(out)
            continue
        for clim_period in PERIODS:
            fname = file_name_bases[clim_period].format(var_name)
            inp, out = os.path.join(args.input_dir, fname), os.path.join(args.output_dir, fname)
            if not os.path.exists(inp):
                raise ValueError('Files for variable ' + var_name + ' are missing')
            if var_name in WINDS and clim_period in wind_pairs:
                if clim_period not in rotated:
                    rotated[clim_period] = dict(zip(WINDS, regrid_lat_lon_wind(*wind_pairs[clim_period], ds_era5, pole, names=WINDS)))
                ds_out = rotated[clim_period][var_name]
            else:
                ds_gcm = ncio.open_dataset(inp)
                ds_out = interp_wrapper(ds_gcm, ds_era5, var_name, i_use_xesmf=settings.i_use_xesmf_regridding,
                                        nan_interp_kernel_radius=nan_interp_kernel_radius,
                                        nan_interp_sharpness=nan_interp_sharpness)
            ncio.to_netcdf(ds_out, out)
            done.append(out)
    return done


if __name__ == '__main__':
    main()
