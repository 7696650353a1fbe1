#!/usr/bin/env python
"""Timing of the default branch's regridding onto point-wise targets (functions.regrid_points, k_regrid_points) from a
192 x 384 global source.  Device events (pgw_profile_get / pgw_timer), every leg warmed up, the legs alternating in one
process, median and min-max of `--reps` (7).  Before EVERY timed leg the output-sized scratch array is overwritten once, untimed,
so that each leg meets the same cache state (the 134 MB of source planes fit the card's last-level cache: a leg that runs
right after another one that read them is up to 0.25 ms faster than the same leg after a large write).  Two cases:
  (a) the 721 x 1440 mesh handed over as 1 038 240 points, 228 planes, float64 and float32: `points`, `regrid` (k_regrid on
      the same mesh: the same output bytes and bits) and `write` (a device memset of the output's bytes, the floor of a
      write-dominated kernel);
  (b) a 1000 x 1000 rotated-pole target (synthetic.rotated_pole_grid), 12 and 228 planes: `points` and `write`.
The kernels' time is the `regrid` profile entry (k_zonal_mean_rows included where pole rows are in use); the host's table
build and the upload of the per-point tables are reported apart (`host_tables_s`, one call on the host clock).
Prints one JSON line per case, storage type and plane count; `--out FILE` appends them to FILE
(profiles/regrid_points_time_<tag>.json).  `--small` runs a 24 x 48 source -> 37 x 72 / 40 x 40, 6-plane rehearsal."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                       # noqa: E402
from pgw4era5_amd import functions as F, synthetic                       # noqa: E402
from pgw4era5_amd.device import default_context                          # noqa: E402


def run(ctx, case, dt, slat, slon, field, tlat2, tlon2, mesh, reps):
    nplanes = int(np.prod(field.shape[:-2]))
    out_bytes = nplanes * tlat2.size * np.dtype(dt).itemsize
    src = ctx.to_device(field, dt)
    t0 = time.perf_counter()
    F.regrid_points(src, slat, slon, tlat2, tlon2).free()                # warm-up; tables, upload and launch on the host clock
    ctx.sync()
    host_s = time.perf_counter() - t0

    def leg_points():
        ctx.profile_reset()
        F.regrid_points(src, slat, slon, tlat2, tlon2).free()
        return ctx.profile_get('regrid')[1]

    def leg_regrid():
        ctx.profile_reset()
        F.regrid_field(src, slat, slon, mesh[0], mesh[1]).free()
        return ctx.profile_get('regrid')[1]

    scratch = ctx.empty((nplanes,) + tlat2.shape, dt)

    def flush():
        ctx._check(ctx.lib.pgw_memset(ctx.handle, scratch.ptr, 0, scratch.nbytes))
        ctx.sync()

    def leg_write():
        ctx.sync()
        ctx.timer_start()
        ctx._check(ctx.lib.pgw_memset(ctx.handle, scratch.ptr, 0, scratch.nbytes))
        return ctx.timer_stop()

    legs = dict(points=leg_points)
    if mesh is not None:
        legs['regrid'] = leg_regrid
    legs['write'] = leg_write
    ctx.profile(True)
    for f in legs.values():
        f()                                                              # warm-up of every leg
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            flush()
            ms[k].append(f())
    ctx.profile(False)
    rec = dict(tool='regrid_points_time', case=case, device=ctx.device_name(), dtype=np.dtype(dt).name,
               source=[len(slat), len(slon)], target=list(tlat2.shape), planes=nplanes, targets=int(tlat2.size),
               out_GB=round(out_bytes / 1e9, 3), host_tables_s=round(host_s, 3))
    if mesh is not None:                                                 # the same bits as k_regrid on the mesh
        one = field.reshape((-1,) + field.shape[-2:])[:2]
        a = F.regrid_points(one, slat, slon, tlat2, tlon2)
        b = F.regrid_field(one, slat, slon, mesh[0], mesh[1])
        rec['same_bits_as_regrid'] = bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))
    for k, v in ms.items():
        rec['%s_ms' % k] = round(float(np.median(v)), 4)
        rec['%s_ms_minmax' % k] = [round(min(v), 4), round(max(v), 4)]
        rec['%s_out_GBps' % k] = round(out_bytes / 1e9 / (float(np.median(v)) / 1e3), 1)
    src.free(); scratch.free()
    print(json.dumps(rec), flush=True)
    return json.dumps(rec)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args(argv)
    shape = dict(nlat_src=24, nlon_src=48, nlat=37, nlon=72, nplev=3, ntime=2) if args.small else \
        dict(nlat_src=192, nlon_src=384, nlat=721, nlon=1440, nplev=19, ntime=12)
    nrot = 40 if args.small else 1000
    ctx = default_context()
    lines = []
    for dt in (np.float64, np.float32):
        g = synthetic.make_gcm_grid_case(seed=4, dtype=dt, **shape)
        la2, lo2 = np.meshgrid(g['targ_lat'], g['targ_lon'], indexing='ij')
        lines.append(run(ctx, 'a: mesh as points', dt, g['src_lat'], g['src_lon'], g['field'], la2, lo2,
                         (g['targ_lat'], g['targ_lon']), args.reps))
        _, _, rlat2, rlon2 = synthetic.rotated_pole_grid(nrot, nrot)
        for field in (g['field'][:, :1], g['field']):                    # 12 and 228 planes
            lines.append(run(ctx, 'b: rotated-pole target', dt, g['src_lat'], g['src_lon'], np.ascontiguousarray(field), rlat2, rlon2,
                             None, args.reps))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
