#!/usr/bin/env python
"""Timing of what settings.delta_grid = 'source_points' adds to step_03: a record of a level delta regridded on the device onto
point-wise targets into its window slot (pgw_points_plan_apply), ua / va rotated in the same launch
(pgw_points_plan_apply_wind).  192 x 384 source onto the 412 x 424 points of a EURO-CORDEX-like rotated grid, one record of 19
planes, float32 source with float32 and float64 output.  Device events (the `regrid` profile entry, which all entries here
are timed under; pgw_timer for the copies), every leg warmed up, the legs alternating in one process, median and min-max of
`--reps` (9, at least 5); before EVERY timed leg the output is overwritten once, untimed, so that each leg meets the same
cache state.  Legs:
  apply     pgw_points_plan_apply of the record into the slot: the profile entry, and the host clock from the call to the end
            of a sync (`apply_call_ms`);
  per_call  pgw_regrid_points on the same source into a float32 array (it has one dtype): the same profile entry - the kernels
            alone - and the host clock, which carries the table upload and its synchronisation (`per_call_call_ms`).  The
            yardstick of `apply`;
  h2d       the copy of the SOURCE record from pinned host memory, what `apply` is fed by;
  write     a device memset of the output's bytes, the floor of a write-dominated kernel;
  wind      pgw_points_plan_apply_wind of a ua / va record pair into two slots;
  composed  pgw_points_plan_apply on ua, on va, then pgw_rotate_pair in place in the source's type: three launches, the
            yardstick of `wind` (float32 -> float32 only: pgw_rotate_pair has one dtype).
The outputs are compared bit for bit with functions.regrid_points / regrid_points_wind, cast on the host, before anything is
timed.  Prints one JSON line per output type; `--out FILE` appends them (profiles/source_points_time_<tag>.json).  `--small`:
a 24 x 48 source, 20 x 22 targets and 3 planes, a rehearsal of the tool."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                       # noqa: E402
from pgw4era5_amd import functions as F, synthetic                       # noqa: E402
from pgw4era5_amd._lib import _dp, _ip                                   # noqa: E402
from pgw4era5_amd.device import PinnedPool, default_context, dtype_tag   # noqa: E402

POLE = (39.25, -162.0)
TABLES = 'lat_lo lat_hi lat_dx lat_Dx lon_lo lon_hi lon_dx lon_Dx oob'.split()


def _stats(rec, name, v, nbytes=None):
    rec['%s_ms' % name] = round(float(np.median(v)), 4)
    rec['%s_ms_minmax' % name] = [round(min(v), 4), round(max(v), 4)]
    if nbytes:
        rec['%s_out_GBps' % name] = round(nbytes / 1e9 / (float(np.median(v)) / 1e3), 1)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def run(ctx, slat, slon, ua, va, tlat, tlon, out_dt, reps, pool):
    S = ua.shape[0]
    src_u, src_v = ctx.to_device(ua), ctx.to_device(va)
    shape = (S,) + tlat.shape
    out_u, out_v = ctx.empty(shape, out_dt), ctx.empty(shape, out_dt)
    out32 = out_u if out_u.dtype == np.float32 else ctx.empty(shape, np.float32)
    plan = F.PointsPlan(slat, slon, tlat, tlon, S, pole=POLE, ctx=ctx)
    cs, sn = F.wind_rotation(ctx.to_device(tlat), ctx.to_device(tlon), *POLE)
    tb = F.regrid_tables(slat, slon, tlat.ravel(), tlon.ravel())
    c = {k: np.ascontiguousarray(tb[k]) for k in TABLES if k != 'oob'}
    c['oob'] = np.ascontiguousarray(tb['lat_oob'] | tb['lon_oob'], dtype=np.int32)
    tabs = [c[k].ctypes.data_as(_ip if c[k].dtype == np.int32 else _dp) for k in TABLES]
    pinned = pool.acquire(src_u.nbytes)
    host = pinned[:src_u.nbytes].view(src_u.dtype).reshape(ua.shape)
    host[...] = ua
    stage = ctx.empty(ua.shape, src_u.dtype)
    # the same bits as the per-call routes, cast on the host
    plan.apply(src_u, out_u)
    same = dict(apply=_same(out_u.numpy(), np.asarray(F.regrid_points(ua, slat, slon, tlat, tlon)).astype(out_dt)))
    plan.apply_wind(src_u, src_v, out_u, out_v)
    want = [np.asarray(x).astype(out_dt) for x in F.regrid_points_wind(ua, va, slat, slon, tlat, tlon, cs, sn)]
    same['wind'] = _same(out_u.numpy(), want[0]) and _same(out_v.numpy(), want[1])
    calls = {}

    def flush():
        for o in (out_u, out_v):
            ctx._check(ctx.lib.pgw_memset(ctx.handle, o.ptr, 0, o.nbytes))
        ctx.sync()

    def timed_call(name, f):
        ctx.profile_reset()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        calls.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return ctx.profile_get('regrid')[1]

    def composed():
        plan.apply(src_u, out_u)
        plan.apply(src_v, out_v)
        ctx._check(ctx.lib.pgw_rotate_pair(ctx.handle, dtype_tag(out_u.dtype), S, tlat.size, out_u.ptr, out_v.ptr, cs.ptr, sn.ptr, 0,
                                           out_u.ptr, out_v.ptr))

    def leg_h2d():
        ctx.sync()
        ctx.timer_start()
        stage.copy_from(host, sync=False)
        return ctx.timer_stop()

    def leg_write():
        ctx.sync()
        ctx.timer_start()
        ctx._check(ctx.lib.pgw_memset(ctx.handle, out_u.ptr, 0, out_u.nbytes))
        return ctx.timer_stop()

    legs = dict(apply=lambda: timed_call('apply', lambda: plan.apply(src_u, out_u)),
                per_call=lambda: timed_call('per_call', lambda: ctx._check(ctx.lib.pgw_regrid_points(
                    ctx.handle, dtype_tag(np.float32), S, len(slat), len(slon), tlat.size, src_u.ptr, *tabs, tb['south_row'],
                    tb['north_row'], out32.ptr))),
                h2d=leg_h2d, write=leg_write,
                wind=lambda: timed_call('wind', lambda: plan.apply_wind(src_u, src_v, out_u, out_v)))
    if out_u.dtype == src_u.dtype:
        legs['composed'] = lambda: timed_call('composed', composed)
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
    rec = dict(tool='source_points_time', device=ctx.device_name(), source=[len(slat), len(slon)], target=list(tlat.shape), S=S,
               src_dtype=src_u.dtype.name, out_dtype=np.dtype(out_dt).name, out_GB=round(out_u.nbytes / 1e9, 4),
               src_GB=round(src_u.nbytes / 1e9, 4), reps=reps, same_bits=same)
    nbytes = dict(apply=out_u.nbytes, per_call=out32.nbytes, h2d=src_u.nbytes, write=out_u.nbytes, wind=2 * out_u.nbytes,
                  composed=2 * out_u.nbytes)
    for k, v in ms.items():
        _stats(rec, k, v, nbytes[k])
    for k, v in calls.items():
        _stats(rec, k + '_call', v)
    rec['apply_over_per_call'] = round(rec['apply_ms'] / rec['per_call_ms'], 3)
    rec['apply_call_over_per_call_call'] = round(rec['apply_call_ms'] / rec['per_call_call_ms'], 3)
    if 'composed' in ms:
        rec['wind_over_composed'] = round(rec['wind_ms'] / rec['composed_ms'], 3)
    pool.release(pinned)
    plan.free()
    for a in {id(x): x for x in (src_u, src_v, out_u, out_v, out32, cs, sn, stage)}.values():
        a.free()
    print(json.dumps(rec), flush=True)
    return json.dumps(rec)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args(argv)
    if args.reps < 5:
        ap.error('--reps must be at least 5')
    shape = dict(nlat_src=24, nlon_src=48, nplev=3, ntime=1) if args.small else dict(nlat_src=192, nlon_src=384, nplev=19, ntime=1)
    _, _, tlat, tlon = synthetic.rotated_pole_grid(*((20, 22) if args.small else (412, 424)))
    ctx = default_context()
    pool = PinnedPool(ctx)
    g = synthetic.make_gcm_grid_case(seed=4, dtype=np.float32, **shape)
    h = synthetic.make_gcm_grid_case(seed=5, dtype=np.float32, **shape)
    ua, va = (np.ascontiguousarray(x['field'].reshape((-1,) + x['field'].shape[-2:])) for x in (g, h))
    lines = [run(ctx, g['src_lat'], g['src_lon'], ua, va, tlat, tlon, out_dt, args.reps, pool) for out_dt in (np.float64, np.float32)]
    pool.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
