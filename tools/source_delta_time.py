#!/usr/bin/env python
"""Timing of what settings.delta_grid = 'source' adds to step_03: a record of a level delta regridded on the device into its
window slot (pgw_regrid_plan_apply) instead of uploaded from a regridded file.  192 x 384 source onto 721 x 1440, one record
of S = 19 and 99 levels, float32 source with float32 and float64 output.  Device events (pgw_profile_get / pgw_timer), every
leg warmed up, the legs alternating in one process, median and min-max of `--reps` (7); before EVERY timed leg the output is
overwritten once, untimed, so that each leg meets the same cache state (tools/regrid_points_time.py).  Legs:
  apply     pgw_regrid_plan_apply of the record: the `regrid` profile entry, and the host clock from the call to the end of a
            sync (`apply_call_ms`);
  bilinear  pgw_regrid_bilinear of the same planes, float32 -> float32 (it has one dtype): the same profile entry - the
            kernels alone - and the host clock, which carries the table upload and its synchronisation (`bilinear_call_ms`);
  h2d       the copy of the regridded record from pinned host memory, what the record window does today;
  write     a device memset of the output's bytes, the floor of a write-dominated kernel.
Then the steady-state time per file of process_file_device at one instant (the bracket does not move, output buffers
reused) on a `--file-grid` NLAT NLON NLEV ERA5 file (default 181 360 40; source 46 x 90, plev19), the DeltaSet fed three
ways: `era5 resident` (step_02's files, all records on the device: the planned call), `era5 window` (the same files through
the host record window: PGW_DELTA_RESIDENT=0) and `source` (records regridded on the device).  Host clock around call + sync.
Prints one JSON line per case; `--out FILE` appends them (profiles/source_delta_time_<tag>.json).  `--small`: a 24 x 48
source onto 37 x 72, S = 3 and 5, a 10 x 10 L20 file - a rehearsal."""
import argparse
import ctypes as C
import datetime as dt
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                       # noqa: E402
from pgw4era5_amd import functions as F, synthetic                       # noqa: E402
from pgw4era5_amd._lib import _dp, _ip                                   # noqa: E402
from pgw4era5_amd.device import PinnedPool, default_context, dtype_tag   # noqa: E402

TABLES = 'lat_lo lat_hi lat_dx lat_Dx lat_oob lon_lo lon_hi lon_dx lon_Dx lon_oob'.split()


def _stats(rec, name, v, nbytes=None):
    rec['%s_ms' % name] = round(float(np.median(v)), 4)
    rec['%s_ms_minmax' % name] = [round(min(v), 4), round(max(v), 4)]
    if nbytes:
        rec['%s_out_GBps' % name] = round(nbytes / 1e9 / (float(np.median(v)) / 1e3), 1)


def regrid_legs(ctx, g, S, out_dt, reps, pool):
    slat, slon, tlat, tlon = g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon']
    rng = np.random.default_rng(S)
    field = rng.normal(size=(S, len(slat), len(slon))).astype(np.float32)
    src = ctx.to_device(field)
    shape = (S, len(tlat), len(tlon))
    out = ctx.empty(shape, out_dt)
    out32 = out if out.dtype == np.float32 else ctx.empty(shape, np.float32)
    plan = F.RegridPlan(slat, slon, tlat, tlon, S, ctx=ctx)
    tb = F.regrid_tables(slat, slon, tlat, tlon)
    c = {k: np.ascontiguousarray(tb[k]) for k in TABLES}
    tabs = [c[k].ctypes.data_as(_ip if c[k].dtype == np.int32 else _dp) for k in TABLES]
    pinned = pool.acquire(out.nbytes)
    host = pinned[:out.nbytes].view(out.dtype).reshape(shape)
    host[...] = 1.0
    calls = {}

    def flush():
        ctx._check(ctx.lib.pgw_memset(ctx.handle, out.ptr, 0, out.nbytes))
        ctx.sync()

    def timed_call(name, f):
        ctx.profile_reset()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        calls.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return ctx.profile_get('regrid')[1]

    def leg_apply():
        return timed_call('apply', lambda: plan.apply(src, out))

    def leg_bilinear():
        return timed_call('bilinear', lambda: ctx._check(ctx.lib.pgw_regrid_bilinear(
            ctx.handle, dtype_tag(np.float32), S, len(slat), len(slon), len(tlat), len(tlon), src.ptr, *tabs, tb['south_row'],
            tb['north_row'], out32.ptr)))

    def leg_h2d():
        ctx.sync()
        ctx.timer_start()
        out.copy_from(host, sync=False)
        return ctx.timer_stop()

    def leg_write():
        ctx.sync()
        ctx.timer_start()
        ctx._check(ctx.lib.pgw_memset(ctx.handle, out.ptr, 0, out.nbytes))
        return ctx.timer_stop()

    legs = dict(apply=leg_apply, bilinear=leg_bilinear, h2d=leg_h2d, write=leg_write)
    ctx.profile(True)
    for f in legs.values():
        f()
    calls.clear()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            flush()
            ms[k].append(f())
    ctx.profile(False)
    rec = dict(tool='source_delta_time', case='record', device=ctx.device_name(), source=[len(slat), len(slon)],
               target=[len(tlat), len(tlon)], S=S, src_dtype='float32', out_dtype=np.dtype(out_dt).name,
               out_GB=round(out.nbytes / 1e9, 3))
    for k, v in ms.items():
        _stats(rec, k, v, out32.nbytes if k == 'bilinear' else out.nbytes)
    for k, v in calls.items():
        _stats(rec, k + '_call', v)
    # the same bits as the one-call route, cast on the host
    plan.apply(src, out)
    want = np.asarray(F.regrid_field(field[:2], slat, slon, tlat, tlon)).astype(out_dt)
    rec['same_bits_as_regrid_field'] = bool(np.array_equal(out.numpy()[:2].view(np.uint8), want.view(np.uint8)))
    pool.release(pinned)
    plan.free()
    for a in {id(x): x for x in (src, out, out32)}.values():
        a.free()
    print(json.dumps(rec), flush=True)
    return json.dumps(rec)


def file_legs(ctx, grid, src_grid, reps):
    from pgw4era5_amd import step_02_preproc_deltas as s2, step_03_apply_to_era as s3, settings as S
    nlat, nlon, nlev = grid
    instant = dt.datetime(2006, 7, 20, 6)
    tmp = tempfile.mkdtemp(prefix='source_delta_time_')
    gcm, regridded, era_dir = (os.path.join(tmp, d) for d in ('gcm', 'regridded', 'era'))
    synthetic.write_gcm_files(gcm, nlat=src_grid[0], nlon=src_grid[1], seed=5, ocean=(30, 44))
    case = synthetic.make_case(nlat, nlon, nlev, seed=3, dtype=np.float32, target_dt=instant)
    path = synthetic.write_case_files(case, era_dir, os.path.join(tmp, 'unused'))
    old_debug, S.i_debug = S.i_debug, -1
    s2.main(['regridding', '-i', gcm, '-o', regridded, '-e', path])
    coeffs = dict(ak=case['era']['ak'], bk=case['era']['bk'], soil1=case['era']['soil1'])
    era = s3._upload_era(ctx, case['era'], np.float32)
    rec = dict(tool='source_delta_time', case='file', device=ctx.device_name(), era=[nlat, nlon, nlev], source=list(src_grid),
               dtype='float32', mode=S.f32_file_mode)
    feeds = (('era5 resident', regridded, 'era5', '1'), ('era5 window', regridded, 'era5', '0'), ('source', gcm, 'source', None))
    sets, outs, ms, n_iter = {}, {}, {k[0]: [] for k in feeds}, {}
    keep = {k: os.environ.get(k) for k in ('PGW_DELTA_GRID', 'PGW_DELTA_RESIDENT')}
    try:
        for name, d, mode, resident in feeds:
            os.environ['PGW_DELTA_GRID'] = mode
            os.environ.pop('PGW_DELTA_RESIDENT', None)
            if resident is not None:
                os.environ['PGW_DELTA_RESIDENT'] = resident
            sets[name] = s3.load_delta_set(ctx, d, np.float32, era5=path)
            s3._DELTASETS.clear()                                        # the next feed loads its own
            outs[name] = {}

        def one(name):
            ctx.sync()
            t0 = time.perf_counter()
            _, info = s3.process_file_device(ctx, era, coeffs, sets[name], instant, True, out=outs[name])
            ctx.sync()
            n_iter[name] = info['n_iter']
            return (time.perf_counter() - t0) * 1e3

        for name in sets:
            one(name); one(name)                                         # warm-up: buffers drawn, records in place, plan made
        for _ in range(reps):
            for name in sets:
                ms[name].append(one(name))
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        S.i_debug = old_debug
    for name, v in ms.items():
        _stats(rec, name.replace(' ', '_'), v)
    rec['n_iter'] = n_iter
    ref = outs['era5 resident']
    rec['same_bits'] = {name: all(bool(np.array_equal(o[k].numpy().view(np.uint8), ref[k].numpy().view(np.uint8))) for k in ref)
                        for name, o in outs.items()}
    for d in sets.values():
        d.free()
    print(json.dumps(rec), flush=True)
    return json.dumps(rec)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--file-grid', type=int, nargs=3, default=None, metavar=('NLAT', 'NLON', 'NLEV'))
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args(argv)
    shape = dict(nlat_src=24, nlon_src=48, nlat=37, nlon=72) if args.small else dict(nlat_src=192, nlon_src=384, nlat=721, nlon=1440)
    levels = (3, 5) if args.small else (19, 99)
    grid = tuple(args.file_grid) if args.file_grid else ((10, 10, 20) if args.small else (181, 360, 40))
    src_grid = (12, 24) if args.small else (46, 90)
    ctx = default_context()
    pool = PinnedPool(ctx)
    g = synthetic.make_gcm_grid_case(seed=4, dtype=np.float32, nplev=1, ntime=1, **shape)
    lines = []
    for S in levels:
        for out_dt in (np.float32, np.float64):
            lines.append(regrid_legs(ctx, g, S, out_dt, args.reps, pool))
    lines.append(file_legs(ctx, grid, src_grid, args.reps))
    pool.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
