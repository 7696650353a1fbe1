#!/usr/bin/env python
"""Timing of the winds' way onto a rotated-pole target grid (`step_02 regridding --rotate_winds`): ua and va of a 192 x 384
global source onto the 412 x 424 points of a EURO-CORDEX-like rotated grid, 12 x 19 planes, float32 and float64.  Three legs:
  fused     pgw_regrid_points_wind (k_zonal_mean_rows where pole rows are in use, k_regrid_points_wind): one launch;
  composed  pgw_regrid_points on ua, on va, then pgw_rotate_pair in place: three launches, two more passes over the outputs;
  write     a device memset of the two outputs' bytes, the floor of a write-dominated kernel.
Device events (the `regrid` profile entry, which all four entries are timed under; pgw_timer for the memset), every leg warmed
up, the legs alternating in one process, median and min-max of `--reps` (9, at least 5).  Before every timed leg an
output-sized scratch array is overwritten once, untimed, so that each leg meets the same cache state.  The tables are built and
uploaded by every call on the host, outside the events.  The legs' outputs are compared bit for bit before anything is timed.
Prints one JSON line per storage type; `--out FILE` appends them to FILE.  `--small`: a 24 x 48 source, 20 x 22 targets and
6 planes, a rehearsal of the tool."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                       # noqa: E402
from pgw4era5_amd import functions as F, synthetic                       # noqa: E402
from pgw4era5_amd.device import default_context, dtype_tag               # noqa: E402

POLE = (39.25, -162.0)


def run(ctx, dt, slat, slon, ua, va, tlat, tlon, reps):
    nplanes = int(np.prod(ua.shape[:-2]))
    out_bytes = 2 * nplanes * tlat.size * np.dtype(dt).itemsize
    d_u, d_v = ctx.to_device(ua, dt), ctx.to_device(va, dt)
    cs, sn = F.wind_rotation(ctx.to_device(tlat), ctx.to_device(tlon), *POLE)

    def fused():
        return F.regrid_points_wind(d_u, d_v, slat, slon, tlat, tlon, cs, sn)

    def composed():
        u, v = F.regrid_points(d_u, slat, slon, tlat, tlon), F.regrid_points(d_v, slat, slon, tlat, tlon)
        ctx._check(ctx.lib.pgw_rotate_pair(ctx.handle, dtype_tag(np.dtype(dt)), nplanes, tlat.size, u.ptr, v.ptr, cs.ptr, sn.ptr, 0,
                                           u.ptr, v.ptr))
        return u, v

    a, b = fused(), composed()                                           # warm-up of both, and the same bits
    same = all(np.array_equal(x.numpy().view(np.uint8), y.numpy().view(np.uint8)) for x, y in zip(a, b))
    for x in a + b:
        x.free()
    scratch = ctx.empty((out_bytes,), np.uint8)

    def profiled(f):
        def leg():
            ctx.profile_reset()
            for x in f():
                x.free()
            return ctx.profile_get('regrid')[1]
        return leg

    def leg_write():
        ctx.sync()
        ctx.timer_start()
        ctx._check(ctx.lib.pgw_memset(ctx.handle, scratch.ptr, 0, scratch.nbytes))
        return ctx.timer_stop()

    legs = dict(fused=profiled(fused), composed=profiled(composed), write=leg_write)
    ctx.profile(True)
    for f in legs.values():
        f()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            ctx._check(ctx.lib.pgw_memset(ctx.handle, scratch.ptr, 0, scratch.nbytes))      # the same cache state for every leg
            ctx.sync()
            ms[k].append(f())
    ctx.profile(False)
    rec = dict(tool='wind_rotate_time', device=ctx.device_name(), dtype=np.dtype(dt).name, source=[len(slat), len(slon)],
               target=list(tlat.shape), planes=nplanes, out_GB=round(out_bytes / 1e9, 3), reps=reps, same_bits=bool(same))
    for k, v in ms.items():
        rec['%s_ms' % k] = round(float(np.median(v)), 4)
        rec['%s_ms_minmax' % k] = [round(min(v), 4), round(max(v), 4)]
        rec['%s_out_GBps' % k] = round(out_bytes / 1e9 / (float(np.median(v)) / 1e3), 1)
    rec['fused_over_composed'] = round(rec['fused_ms'] / rec['composed_ms'], 3)
    for x in (d_u, d_v, cs, sn, scratch):
        x.free()
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
    shape = dict(nlat_src=24, nlon_src=48, nplev=3, ntime=2) if args.small else dict(nlat_src=192, nlon_src=384, nplev=19, ntime=12)
    _, _, tlat, tlon = synthetic.rotated_pole_grid(*((20, 22) if args.small else (412, 424)))
    ctx = default_context()
    lines = []
    for dt in (np.float32, np.float64):
        g = synthetic.make_gcm_grid_case(seed=4, dtype=dt, **shape)
        h = synthetic.make_gcm_grid_case(seed=5, dtype=dt, **shape)
        lines.append(run(ctx, dt, g['src_lat'], g['src_lon'], g['field'], h['field'], tlat, tlon, args.reps))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
