"""
Delta check of step_03's output: the applied change of T, RH, U and V on EVERY level of the deltas.

step_03 adds the `ta`, `hur`, `ua` and `va` deltas on model levels at the ERA5 pressures and then moves the surface
pressure, so every model level of the written file sits at another pressure (the reference's `i_reinterp = 1` exists to
repair this).  This module asks what a regional model sees at fixed pressure: on the plev axis of the deltas,

    error_X(p) = (X_pgw(p) - X_era(p)) - delta_X(p)        where p < ps_hist, NaN elsewhere

with X(p) = interp_extrap_1d(ln(akm + PS * bkm), X, ln p, 'nan') (reference functions.py:511-580), RH =
specific_to_relative_humidity(QV, pa, T) (:107-116) and delta_X, ps_hist interpolated in time like load_delta (:195-303),
every variable on its own time axis.  At and below ps_hist step_03 applies the surface delta (replace_delta_sfc), so the
level's delta is no yardstick there.  Arithmetic is float64 on the stored values whatever the files' dtypes (a diagnostic,
not part of the drop-in path).  No counterpart in the reference.

One launch of `pgw_state_on_plev` and one `pgw_level_stats` per file; files are processed one after the other.

    python -m pgw4era5_amd.check_deltas -i ERA_IN -g PGW_DIR -d DELTA_DIR -o CHECK_DIR -f 2006080200 -l 2006080300 -H 3
"""
import os

import numpy as np

from . import settings as S
from .check_geopot import _same_grid, era_steps, table_from_partials

CHECK_PREFIX = 'deltacheck_'
VARS = ('ta', 'hur', 'ua', 'va')
UNITS = dict(ta='K', hur='%', ua='m s-1', va='m s-1')


def check_path(out_dir, era_file_path):
    """`deltacheck_{file name}` in `out_dir`."""
    return os.path.join(out_dir, CHECK_PREFIX + os.path.basename(era_file_path))


def format_table(table, unit):
    """One variable's table (`check_geopot.table_from_partials` of its error rows) as text, one row per level in the order
    of the delta files, in the variable's own unit."""
    u = '[%s]' % unit
    lines = ['%10s %9s %16s %16s %16s' % ('plev [Pa]', 'n_valid', 'mean ' + u, 'rms ' + u, 'max ' + u)]
    for i, p in enumerate(table['plev']):
        lines.append('%10.1f %9d %16.8g %16.8g %16.8g' % (p, table['n_valid'][i], table['mean'][i], table['rms'][i], table['max'][i]))
    return '\n'.join(lines)


def check_file(inp_era_file_path, pgw_era_file_path, delta_input_dir, era_step_dt, out_path):
    """The check of one file pair: `inp_era_file_path` (what step_03 read) and `pgw_era_file_path` (what it wrote), with the
    ta, hur, ua, va and ps_hist records of `delta_input_dir` (through `load_delta_set`, so also deltas on the GCM's grid with
    settings.delta_grid = 'source') interpolated to `era_step_dt`.  Writes the NetCDF-3 file `out_path` with
    {ta,hur,ua,va}_change and {ta,hur,ua,va}_error (time, plev, lat, lon - or the horizontal dimensions of a file with 2-D
    lat / lon or a cell list) float64 and returns dict variable -> per-level table of the error (`table_from_partials`).
    ValueError when the two files differ in grid or level count."""
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

    names = dict(PS=(vm['ps'], dims3), T=(vm['ta'], dims4), QV=(vm['hus'], dims4), U=(vm['ua'], dims4), V=(vm['va'], dims4))
    a = {k: get(era_file, n, d) for k, (n, d) in names.items()}
    b = {k: get(pgw_file, n, d) for k, (n, d) in names.items()}
    ak, bk = (np.asarray(era_file[k].values, dtype=np.float64) for k in ('ak', 'bk'))
    if b['PS'].shape != a['PS'].shape:
        raise ValueError('the PGW file is on another grid: PS %s, input file %s' % (b['PS'].shape, a['PS'].shape))
    for k in ('T', 'QV', 'U', 'V'):
        if b[k].shape != a['T'].shape or a[k].shape != a['T'].shape:
            raise ValueError('the PGW file has other levels or another grid: %s %s, input file T %s' % (k, b[k].shape, a['T'].shape))
    if a['T'].shape[1] != len(ak) - 1:
        raise ValueError('%d model levels, but ak and bk describe %d' % (a['T'].shape[1], len(ak) - 1))
    _same_grid(era_file, pgw_file)
    nt, nlat, nlon = a['PS'].shape
    if nt != 1:
        raise ValueError('Time dimension of input files is inconsistent!')          # one instant per file, like step_03
    ctx = default_context()
    deltas = s3.load_delta_set(ctx, delta_input_dir, a['T'].dtype, era5=(era_file, inp_era_file_path))
    plev = F.check_plev(deltas.plev, most=128)
    sz = (1, len(plev), nlat, nlon)
    pairs = {}
    for var in VARS + ('ps_hist',):
        rb, ra, x_hi, x_new = deltas.pair(var, era_step_dt, None)
        want = sz[2:] if var == 'ps_hist' else sz[1:]
        if tuple(rb.shape) != want:
            raise ValueError('the %s delta %s is not on the grid of the ERA5 file %s' % (var, tuple(rb.shape), want))
        shape = (1,) + want
        pairs[var] = (rb.view(shape), ra.view(shape), x_hi, x_new)
    dev = {k: ctx.to_device(v, v.dtype) for k, v in a.items()}
    dev.update({k + '_b': ctx.to_device(v, v.dtype) for k, v in b.items()})
    change, error = F.state_change_on_plev(dev['PS'], dev['T'], dev['QV'], dev['U'], dev['V'], dev['PS_b'], dev['T_b'], dev['QV_b'],
                                           dev['U_b'], dev['V_b'], ak, bk, plev, deltas=pairs)
    stats = F.level_stats(error.view((4 * len(plev), nlat * nlon)))
    tables = {}
    for i, var in enumerate(VARS):
        rows = slice(i * len(plev), (i + 1) * len(plev))
        tables[var] = table_from_partials(plev, stats['count'][rows], stats['sum'][rows], stats['sumsq'][rows], stats['maxabs'][rows])
    ds = ncio.Dataset()
    dims = (S.TIME_ERA, S.PLEV_GCM) + H
    for d in (S.TIME_ERA,) + H:
        if d in era_file and era_file[d].dims == (d,):
            ds[d] = ncio.Field(era_file[d].values, (d,), {}, era_file[d].attrs)
    ds[S.PLEV_GCM] = ncio.Field(plev, (S.PLEV_GCM,), {}, dict(units='Pa'))
    coords = {d: ds[d].values for d in dims if d in ds}
    change_h, error_h = change.numpy(), error.numpy()
    for i, var in enumerate(VARS):
        ds[var + '_change'] = ncio.Field(s3._as_file(change_h[i], H), dims, coords, dict(
            units=UNITS[var], long_name='change of %s of the PGW state against the ERA5 state on pressure levels' % var))
        ds[var + '_error'] = ncio.Field(s3._as_file(error_h[i], H), dims, coords, dict(
            units=UNITS[var], long_name='%s_change - %s climate delta above ps_hist' % (var, var)))
    ncio.to_netcdf(ds, out_path)
    for v in list(dev.values()) + [change, error]:
        v.free()
    return tables


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(description='Delta check of step_03 output: change of T, RH, U, V of the PGW state on every level '
                                            'of the deltas (date arguments and file names as step_03_apply_to_era).')
    p.add_argument('-i', '--input_dir', type=str, default=None, help='directory with the ERA5 files step_03 read')
    p.add_argument('-g', '--pgw_dir', type=str, default=None, help='directory with the files step_03 wrote')
    p.add_argument('-d', '--delta_input_dir', type=str, default=None, help='directory with the climate deltas')
    p.add_argument('-o', '--output_dir', type=str, default=None, help='directory for the deltacheck_* files')
    p.add_argument('-f', '--first_era_step', type=str, default='2006080200', help='first time step, YYYYMMDDHH')
    p.add_argument('-l', '--last_era_step', type=str, default='2006080300', help='last time step (inclusive), YYYYMMDDHH')
    p.add_argument('-H', '--hour_inc_step', type=int, default=3, help='hours between time steps')
    p.add_argument('--delta_grid', type=str, default=None, choices=('era5', 'source', 'source_points'),
                   help="grid of the delta files: 'era5' (step_02 wrote them), 'source' (the GCM's grid, mesh files) or "
                        "'source_points' (the GCM's grid, files of any layout); default settings.delta_grid")
    p.add_argument('--rotate_winds', type=str, nargs='?', const='auto', default=None, metavar='auto|POLE_LAT,POLE_LON',
                   help="as step_03's flag: the run rotated the ua / va deltas onto the file's rotated grid (--delta_grid source_points)")
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
    results = []
    # what step_03's command line sets (delta_grid_mode reads them)
    handed = {k: v for k, v in (('PGW_DELTA_GRID', args.delta_grid), ('PGW_ROTATE_WINDS', args.rotate_winds)) if v is not None}
    before = {k: os.environ.get(k) for k in handed}
    os.environ.update(handed)
    try:
        for job in file_jobs(args):
            tables = check_file(**job)
            print('{}: error = (X_pgw - X_era) - delta above ps_hist, written to {}'.format(job['pgw_era_file_path'], job['out_path']))
            for var in VARS:
                print('%s_error' % var)
                print(format_table(tables[var], UNITS[var]))
            results.append(tables)
    finally:
        for k, v in before.items():
            os.environ.pop(k)
            if v is not None:
                os.environ[k] = v
    return results


if __name__ == '__main__':
    _cli()
