"""
Hydrostatic check of step_03's output: the geopotential change of the PGW state on EVERY level of the zg delta.

step_03 moves the surface pressure until the geopotential change at one level, `p_ref`, matches the GCM's zg delta
(reference step_03_apply_to_era.py:189-319); the only figure a run prints is the maximum error at that level.  This module
evaluates the loop's `phi_ref_error` (:289, 298) on all levels of `zg_delta.nc`, on the files step_03 wrote - what goes into
the regional model:

    phi_error(p) = (phi_pgw(p) - phi_era(p)) - g * zg_delta(p)

with phi(p) = integ_geopot(ak + PS * bk, FIS, T, QV, level1, p_ref=p) (reference functions.py:128-189) and zg_delta
interpolated in time like load_delta (:195-303).  Where a level lies below a column's surface half level the reference's
integ_geopot raises; here the value is NaN and the column does not count for that level.  Arithmetic is float64 on the stored
values whatever the files' dtypes (the float32 roundings of the reference-dtype mode are not reproduced: a diagnostic, not part
of the drop-in path).  No counterpart in the reference.

One launch of `pgw_geopot_on_plev` per output field and one `pgw_level_stats` per file; files are processed one after the other.

    python -m pgw4era5_amd.check_geopot -i ERA_IN -g PGW_DIR -d DELTA_DIR -o CHECK_DIR -f 2006080200 -l 2006080300 -H 3
"""
import datetime as _dt
import os

import numpy as np

from . import settings as S
from .constants import CON_G

CHECK_PREFIX = 'zgcheck_'


def check_path(out_dir, era_file_path):
    """`zgcheck_{file name}` in `out_dir`."""
    return os.path.join(out_dir, CHECK_PREFIX + os.path.basename(era_file_path))


def table_from_partials(plev, count, total, sumsq, maxabs):
    """The per-level table from the NaN-skipping partials of phi_error (count, sum, sum of squares, max |x| per level):
    dict of vectors plev, n_valid, mean, rms, max [m2 s-2] and mean_m, rms_m, max_m [m] (divided by g).  A level without a
    valid column has NaN statistics and n_valid 0."""
    n = np.asarray(count, dtype=np.int64)
    total, sumsq, maxabs = (np.asarray(x, dtype=np.float64) for x in (total, sumsq, maxabs))
    with np.errstate(invalid='ignore', divide='ignore'):
        nf = np.where(n > 0, n, 1).astype(np.float64)
        mean = np.where(n > 0, total / nf, np.nan)
        rms = np.where(n > 0, np.sqrt(sumsq / nf), np.nan)
        mx = np.where(n > 0, maxabs, np.nan)
    return dict(plev=np.asarray(plev, dtype=np.float64), n_valid=n, mean=mean, rms=rms, max=mx,
                mean_m=mean / CON_G, rms_m=rms / CON_G, max_m=mx / CON_G)


def format_table(table, p_ref=None, thresh=None):
    """The table as text, one row per level in the order of the zg file; the `p_ref` row is marked and its maximum compared
    with `thresh` (settings.p_ref_inp, settings.thresh_phi_ref_max_error by default)."""
    p_ref = S.p_ref_inp if p_ref is None else p_ref
    thresh = S.thresh_phi_ref_max_error if thresh is None else thresh
    lines = ['%10s %9s %13s %13s %13s %11s %11s %11s' % ('plev [Pa]', 'n_valid', 'mean [m2/s2]', 'rms [m2/s2]', 'max [m2/s2]',
                                                         'mean [m]', 'rms [m]', 'max [m]')]
    for i, p in enumerate(table['plev']):
        row = '%10.1f %9d %13.6g %13.6g %13.6g %11.5g %11.5g %11.5g' % (
            p, table['n_valid'][i], table['mean'][i], table['rms'][i], table['max'][i], table['mean_m'][i], table['rms_m'][i],
            table['max_m'][i])
        if p_ref is not None and p_ref != 'local' and float(p) == float(p_ref):
            ok = table['max'][i] <= thresh
            row += '  <- p_ref: max %s thresh_phi_ref_max_error = %g' % ('<=' if ok else '>', thresh)
        lines.append(row)
    return '\n'.join(lines)


def _same_grid(era_file, pgw_file):
    for d in (S.TIME_ERA, S.LAT_ERA, S.LON_ERA):
        if d in era_file and d in pgw_file:
            a, b = np.asarray(era_file[d].values), np.asarray(pgw_file[d].values)
            if a.shape != b.shape or (d != S.TIME_ERA and not np.array_equal(a, b)):
                raise ValueError('%s of the PGW file differs from the input file' % d)


def check_file(inp_era_file_path, pgw_era_file_path, delta_input_dir, era_step_dt, out_path):
    """The check of one file pair: `inp_era_file_path` (what step_03 read) and `pgw_era_file_path` (what it wrote), with the
    zg delta of `delta_input_dir` interpolated to `era_step_dt` on the zg file's own plev and time axis.  Writes the NetCDF-3
    file `out_path` with phi_change = phi_pgw - phi_era, phi_delta = g * zg_delta and phi_error = phi_change - phi_delta
    (time, plev, lat, lon - or the horizontal dimensions of a file with 2-D lat / lon or a cell list) float64 [m2 s-2] and
    returns the per-level table (`table_from_partials`).  ValueError when the two files differ in grid or level count."""
    from . import ncio
    from . import functions as F
    from . import step_03_apply_to_era as s3
    from .device import default_context
    vm = S.var_name_map
    era_file = ncio.open_dataset(inp_era_file_path, decode_times=False)
    pgw_file = ncio.open_dataset(pgw_era_file_path, decode_times=False)
    H = s3.era_layout(era_file)                             # (lat, lon), or the dimensions of 2-D lat / lon, or (cell,)
    hdims = s3.layout_dims(H)
    dims3, dims4 = hdims['d3'], hdims['d4']

    def get(ds, name, dims):
        if not s3.is_mesh(H):
            s3._check_dims(name, ds[name], dims)
        v = np.asarray(ds[name].transpose(*dims).values)
        return s3._as_grid(np.ascontiguousarray(v, dtype=np.float64 if v.dtype.itemsize == 8 else np.float32), H)

    a = dict(PS=get(era_file, vm['ps'], dims3), FIS=get(era_file, vm['zgs'], dims3), T=get(era_file, vm['ta'], dims4),
             QV=get(era_file, vm['hus'], dims4))
    b = dict(PS=get(pgw_file, vm['ps'], dims3), T=get(pgw_file, vm['ta'], dims4), QV=get(pgw_file, vm['hus'], dims4))
    ak, bk = (np.asarray(era_file[k].values, dtype=np.float64) for k in ('ak', 'bk'))
    if b['PS'].shape != a['PS'].shape:
        raise ValueError('the PGW file is on another grid: PS %s, input file %s' % (b['PS'].shape, a['PS'].shape))
    if b['T'].shape != a['T'].shape or b['QV'].shape != a['T'].shape:
        raise ValueError('the PGW file has other levels or another grid: T %s, input file %s' % (b['T'].shape, a['T'].shape))
    if a['T'].shape[1] != len(ak) - 1:
        raise ValueError('%d model levels, but ak and bk describe %d' % (a['T'].shape[1], len(ak) - 1))
    _same_grid(era_file, pgw_file)
    nt, nlat, nlon = a['PS'].shape
    if nt != 1:
        raise ValueError('Time dimension of input files is inconsistent!')          # one instant per file, like step_03
    ctx = default_context()
    deltas = s3.load_delta_set(ctx, delta_input_dir, a['T'].dtype, era5=(era_file, inp_era_file_path))
    plev = F.check_plev(deltas.plev_zg)
    zb, za, x_hi, x_new = deltas.pair('zg', era_step_dt, None)
    sz = (1, len(plev), nlat, nlon)
    if tuple(zb.shape) != sz[1:]:
        raise ValueError('the zg delta %s is not on the grid of the ERA5 file %s' % (tuple(zb.shape), sz[1:]))
    dzg = (zb.view(sz), za.view(sz), x_hi, x_new)
    dev = {k: ctx.to_device(v, v.dtype) for k, v in a.items()}
    dev.update({k + '_b': ctx.to_device(v, v.dtype) for k, v in b.items()})
    states = (dev['PS'], dev['T'], dev['QV'], dev['PS_b'], dev['T_b'], dev['QV_b'], dev['FIS'], ak, bk, plev)
    change = F.geopot_change_on_plev(*states)
    error = F.geopot_change_on_plev(*states, dzg=dzg)
    stats = F.level_stats(error.view((len(plev), nlat * nlon)))
    table = table_from_partials(plev, stats['count'], stats['sum'], stats['sumsq'], stats['maxabs'])
    # g * zg_delta for the file: the time interpolation of the kernel (functions.py:288-292) on the host copy of two records
    zb_h = zb.numpy().astype(np.float64)
    if x_hi == 0.0:
        delta = zb_h * CON_G
    else:
        delta = ((za.numpy().astype(np.float64) - zb_h) / x_hi * x_new + zb_h) * CON_G
    ds = ncio.Dataset()
    dims = (S.TIME_ERA, S.PLEV_GCM) + H
    for d in (S.TIME_ERA,) + H:
        if d in era_file and era_file[d].dims == (d,):
            ds[d] = ncio.Field(era_file[d].values, (d,), {}, era_file[d].attrs)
    ds[S.PLEV_GCM] = ncio.Field(plev, (S.PLEV_GCM,), {}, dict(units='Pa'))
    coords = {d: ds[d].values for d in dims if d in ds}
    names = dict(phi_change='geopotential change of the PGW state against the ERA5 state',
                 phi_delta='g times the zg climate delta', phi_error='phi_change - phi_delta')
    for name, arr in (('phi_change', change.numpy()), ('phi_delta', delta.reshape(sz)), ('phi_error', error.numpy())):
        ds[name] = ncio.Field(s3._as_file(arr, H), dims, coords, dict(units='m2 s-2', long_name=names[name]))
    ncio.to_netcdf(ds, out_path)
    for v in list(dev.values()) + [change, error]:
        v.free()
    return table


def era_steps(first_era_step, last_era_step, hour_inc_step):
    """The time steps of step_03's command line (np.arange(first, last + inc, inc), reference step_03:594-596)."""
    first = _dt.datetime.strptime(first_era_step, '%Y%m%d%H')
    last = _dt.datetime.strptime(last_era_step, '%Y%m%d%H')
    inc = _dt.timedelta(hours=hour_inc_step)
    steps, t = [], first
    while t < last + inc:
        steps.append(t)
        t += inc
    return steps


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(description='Hydrostatic check of step_03 output: geopotential change of the PGW state on every '
                                            'level of the zg delta (date arguments and file names as step_03_apply_to_era).')
    p.add_argument('-i', '--input_dir', type=str, default=None, help='directory with the ERA5 files step_03 read')
    p.add_argument('-g', '--pgw_dir', type=str, default=None, help='directory with the files step_03 wrote')
    p.add_argument('-d', '--delta_input_dir', type=str, default=None, help='directory with the climate deltas (zg_delta.nc)')
    p.add_argument('-o', '--output_dir', type=str, default=None, help='directory for the zgcheck_* files')
    p.add_argument('-f', '--first_era_step', type=str, default='2006080200', help='first time step, YYYYMMDDHH')
    p.add_argument('-l', '--last_era_step', type=str, default='2006080300', help='last time step (inclusive), YYYYMMDDHH')
    p.add_argument('-H', '--hour_inc_step', type=int, default=3, help='hours between time steps')
    args = p.parse_args(argv)
    for flag, val in (('-i', args.input_dir), ('-g', args.pgw_dir), ('-d', args.delta_input_dir), ('-o', args.output_dir)):
        if val is None:
            raise ValueError('Directory (%s) is required.' % flag)
    return args


def file_jobs(args):
    """One dict of check_file arguments per time step (file-name rule of step_03: settings.era5_file_name_base)."""
    jobs = []
    for s in era_steps(args.first_era_step, args.last_era_step, args.hour_inc_step):
        name = S.era5_file_name_base.format(s)
        jobs.append(dict(inp_era_file_path=os.path.join(args.input_dir, name), pgw_era_file_path=os.path.join(args.pgw_dir, name),
                         delta_input_dir=args.delta_input_dir, era_step_dt=s, out_path=check_path(args.output_dir, name)))
    return jobs


def _cli(argv=None):
    args = parse_args(argv)
    os.makedirs(args.output_dir, exist_ok=True)
    tables = []
    for job in file_jobs(args):
        table = check_file(**job)
        print('{}: phi_error = (phi_pgw - phi_era) - g * zg_delta, written to {}'.format(job['pgw_era_file_path'], job['out_path']))
        print(format_table(table))
        tables.append(table)
    return tables


if __name__ == '__main__':
    _cli()
