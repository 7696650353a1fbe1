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

Not in the reference either: `--source_winds [auto | POLE_LAT,POLE_LON | geographic]` for settings.i_use_xesmf_regridding = 1
and deltas from a regional model on a rotated-pole grid, whose stored ua / va are GRID-RELATIVE on the SOURCE grid: ua and va of
each period are turned to geographic, regridded together and - with `--rotate_winds` - rotated onto a rotated target's
directions, in one launch (functions.regrid_lat_lon_source_wind).  `geographic` declares the source winds eastward /
northward, for `--rotate_winds` with the setting on.  Off by default; with it off nothing about a run differs.
"""
import argparse
import os
from pathlib import Path

import numpy as np

from . import ncio
from .functions import (filter_data, interp_wrapper, regrid_lat_lon_wind, regrid_lat_lon_source_wind, check_wind_pair, rotated_pole_of,
                        _Target)
from . import settings
from .settings import file_name_bases, nan_interp_kernel_radius, nan_interp_sharpness, LAT_ERA, LON_ERA, LAT_GCM, LON_GCM

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
    p.add_argument('--source_winds', type=str, nargs='?', const='auto', default=None, metavar='auto|POLE_LAT,POLE_LON|geographic',
                   help='regridding with settings.i_use_xesmf_regridding = 1 from a rotated-pole source grid: the ua / va of the '
                        'input files are grid-relative components (along rlon / rlat of the source grid) and are turned to '
                        "eastward / northward before they are regridded.  auto (the value when none is given): the pole is taken "
                        "from the ua input file's rotated_latitude_longitude mapping; or the geographic position of the source "
                        "grid's north pole in degrees; geographic: the input winds are eastward / northward (for --rotate_winds "
                        'with the setting on).  Default: off')
    return p


def wind_pole(rotate_winds, ds_era5, flag='--rotate_winds', var_name=None, file='target file'):
    """The value of `--rotate_winds` -> (pole_lat, pole_lon): `auto` from the rotated mapping of the target file (rotated_pole_of),
    else POLE_LAT,POLE_LON parsed and checked.  ValueError naming the cause.  Also the rule of step_03's --rotate_winds, and -
    under the name `flag`, on the variable `var_name` of the `file` - of --source_winds."""
    if rotate_winds == 'auto':
        return rotated_pole_of(ds_era5, settings.var_name_map['ua'] if var_name is None else var_name, flag, file)
    try:
        lat, lon = (float(x) for x in rotate_winds.split(','))
    except ValueError:
        raise ValueError("%s takes 'auto' or POLE_LAT,POLE_LON in degrees, got %r" % (flag, rotate_winds)) from None
    if not (-90.0 <= lat <= 90.0 and -360.0 <= lon <= 360.0):
        raise ValueError('%s: a pole at latitude %r, longitude %r is not a position in degrees' % (flag, lat, lon))
    return (lat, lon)


def _wind_plan(args, var_names, ds_era5):
    """Everything `--rotate_winds` and `--source_winds` can object to, before a file is written -> (source pole, target pole,
    {period: (ds_ua, ds_va)}), the input files opened; a pole is None where that side's winds are geographic.  ValueError
    naming the cause."""
    source = args.source_winds is not None
    flag = '--rotate_winds' if args.rotate_winds is not None else '--source_winds'
    if args.processing_step == 'smoothing':
        raise ValueError('%s belongs to the regridding step: smoothing runs on the GCM grid, where the winds are %s'
                         % (flag, 'geographic' if flag == '--rotate_winds' else 'left as they are'))
    if settings.i_use_xesmf_regridding and not source:
        raise ValueError('--rotate_winds with settings.i_use_xesmf_regridding = 1 is not built: a curvilinear or rotated source '
                         'grid may carry grid-relative winds of its own, which would have to be turned to geographic first - '
                         'say what the source winds follow with --source_winds [auto | POLE_LAT,POLE_LON | geographic]')
    if source and not settings.i_use_xesmf_regridding:
        raise ValueError('--source_winds needs settings.i_use_xesmf_regridding = 1: in the default branch the source is a '
                         'lat-lon mesh, whose winds are geographic already')
    if source and args.source_winds == 'geographic' and args.rotate_winds is None:
        raise ValueError('--source_winds geographic without --rotate_winds: geographic winds onto geographic directions, there '
                         'is nothing to rotate')
    if args.rotate_winds is not None:
        tg = _Target.of(ds_era5[LAT_ERA], ds_era5[LON_ERA])
        if not tg.points:
            raise ValueError('--rotate_winds: the target file has 1-D lat / lon axes - the winds of a lat-lon mesh are geographic '
                             'already, there is nothing to rotate')
        if source and tg.lat.ndim != 2:
            raise ValueError('--rotate_winds with --source_winds: the target file needs 2-D lat / lon, got %d-D' % tg.lat.ndim)
    have = [w in var_names for w in WINDS]
    if have[0] != have[1] or (source and not have[0]):
        raise ValueError('%s needs ua and va together: -v lists %s' % (flag, 'neither' if not (have[0] or have[1]) else
                         '%s without %s' % ((WINDS[0], WINDS[1]) if have[0] else (WINDS[1], WINDS[0]))))
    pole = wind_pole(args.rotate_winds, ds_era5) if args.rotate_winds is not None else None
    pairs = {}
    if have[0]:
        for period in PERIODS:
            paths = [os.path.join(args.input_dir, file_name_bases[period].format(w)) for w in WINDS]
            for w, path in zip(WINDS, paths):
                if not os.path.exists(path):
                    raise ValueError('Files for variable ' + w + ' are missing')
            pairs[period] = tuple(ncio.open_dataset(path) for path in paths)
            check_wind_pair(*pairs[period], names=WINDS, flag=flag, source_winds=source)
    source_pole = None
    if source and args.source_winds != 'geographic':
        ds_ua = pairs[PERIODS[0]][0]
        source_pole = wind_pole(args.source_winds, ds_ua, '--source_winds', WINDS[0], 'source ua file')
        if any(np.ndim(ds[c].values) != 2 for ds in pairs[PERIODS[0]] for c in (LAT_GCM, LON_GCM)):
            raise ValueError('--source_winds %s: the source files have 1-D lat / lon axes - the winds of a lat-lon mesh are '
                             'geographic already; a pole needs 2-D source coordinates' % args.source_winds)
    return source_pole, pole, pairs


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
    flagged = args.rotate_winds is not None or args.source_winds is not None
    source_pole, pole, wind_pairs = _wind_plan(args, var_names, ds_era5) if flagged else (None, None, {})
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
                    if args.source_winds is not None:
                        pair = regrid_lat_lon_source_wind(*wind_pairs[clim_period], ds_era5, source_pole, pole, names=WINDS)
                    else:
                        pair = regrid_lat_lon_wind(*wind_pairs[clim_period], ds_era5, pole, names=WINDS)
                    rotated[clim_period] = dict(zip(WINDS, pair))
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
