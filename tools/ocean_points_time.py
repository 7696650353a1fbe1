#!/usr/bin/env python
"""Timing of the ocean-grid interpolation onto point-wise targets (functions.gauss_interp_points: pgw_ocean_targets,
pgw_gauss_interp_points) beside the mesh path (functions.gauss_interp_fields, k_gauss_interp) on the same targets: the
721 x 1440 mesh and the 404 x 802 ocean source of tests/test_ocean_interp.py's full-size leg, twelve months, R = 1000 km,
sharpness 4.  Each run handles the mesh three ways, alternating in one process, `--reps` (5) times after a warm-up of every
leg:
  mesh      gauss_interp_fields; kernel = the `gauss_interp` profile entry (k_gauss_interp on the host-tiled targets);
  rowmajor  the meshgrid handed to gauss_interp_points as (721, 1440) arrays;
  permuted  the same targets in a random permutation.
For the two point legs the C entries are also called on their own, on device arrays: `targets_ms` is pgw_ocean_targets
between pgw_timer_start / _stop, `entry_ms` pgw_gauss_interp_points the same way, `gather_ms` its `gauss_interp` profile
entry (k_gauss_points) and `key_order_ms` = entry - gather (memset, k_gauss_keys, k_gauss_scan, k_gauss_scatter and the
gaps between the five launches).  `wall_s` is the whole function call on the host clock, result on the host.
Prints one JSON line; `--out FILE` appends it to FILE (profiles/ocean_points_time_<tag>.json).  `--small` is a 40 x 60 source
-> 37 x 72 rehearsal."""
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args(argv)
    if args.small:
        oc = synthetic.make_ocean_grid_case(nj=40, ni=60, ntime=12, seed=6)
        nlat, nlon = 37, 72
        land = np.zeros((nlat, nlon)); land[20:24, 10:16] = 1.0
    else:
        oc = synthetic.make_ocean_grid_case(nj=404, ni=802, ntime=12, seed=6, land_patches=6)
        nlat, nlon = 721, 1440
        land = np.zeros((nlat, nlon)); land[400:430, 200:260] = 1.0
    R, s = 1.0e6, 4.0
    lat, lon = np.linspace(-90.0, 90.0, nlat), np.arange(nlon) * (360.0 / nlon)
    lat2, lon2 = np.meshgrid(lat, lon, indexing='ij')
    perm = np.random.default_rng(0).permutation(lat2.size)
    src = (oc['latitude'], oc['longitude'], list(oc['values']), R, s)
    ctx = default_context()
    f64 = np.dtype('float64')
    cloud = F._OceanCloud(ctx, oc['latitude'], oc['longitude'], list(oc['values']), R)
    ntarg = lat2.size
    dev = {}
    for name, idx in (('rowmajor', np.arange(ntarg)), ('permuted', perm)):
        dev[name] = dict(lat=ctx.to_device(np.ascontiguousarray(lat2.ravel()[idx]), f64),
                         lon=ctx.to_device(np.ascontiguousarray(lon2.ravel()[idx]), f64),
                         land=ctx.to_device(np.ascontiguousarray(land.ravel()[idx]), f64))
    d_tx, d_ty = ctx.empty((ntarg,), f64), ctx.empty((ntarg,), f64)
    d_out = ctx.empty((12, ntarg), f64)
    results = {}

    def leg_mesh():
        ctx.profile_reset()
        t0 = time.perf_counter()
        results['mesh'] = F.gauss_interp_fields(land, lat, lon, *src)
        return dict(wall_s=time.perf_counter() - t0, kernel_ms=ctx.profile_get('gauss_interp')[1])

    def leg_points(name, idx):
        def leg():
            d = dev[name]
            ctx.sync()
            ctx.timer_start()
            ctx._check(ctx.lib.pgw_ocean_targets(ctx.handle, ntarg, d['lat'].ptr, d['lon'].ptr, d['land'].ptr, d_tx.ptr, d_ty.ptr))
            targets = ctx.timer_stop()
            ctx.profile_reset()
            ctx.timer_start()
            ctx._check(ctx.lib.pgw_gauss_interp_points(ctx.handle, ntarg, d_tx.ptr, d_ty.ptr, cloud.ncx, cloud.ncy, cloud.x0,
                                                       cloud.y0, cloud.h, cloud.d_cs.ptr, cloud.nsrc, cloud.d_sx.ptr, cloud.d_sy.ptr,
                                                       cloud.d_sv.ptr, 12, R, s, d_out.ptr))
            entry = ctx.timer_stop()
            gather = ctx.profile_get('gauss_interp')[1]
            t0 = time.perf_counter()
            shape = lat2.shape if name == 'rowmajor' else (ntarg,)
            results[name] = F.gauss_interp_points(land.ravel()[idx].reshape(shape), lat2.ravel()[idx].reshape(shape),
                                                  lon2.ravel()[idx].reshape(shape), *src)
            return dict(wall_s=time.perf_counter() - t0, targets_ms=targets, entry_ms=entry, gather_ms=gather,
                        key_order_ms=entry - gather)
        return leg

    legs = dict(mesh=leg_mesh, rowmajor=leg_points('rowmajor', np.arange(ntarg)), permuted=leg_points('permuted', perm))
    ctx.profile(True)
    for f in legs.values():
        f()                                                              # warm-up of every leg
    runs = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, f in legs.items():
            runs[k].append(f())
    ctx.profile(False)
    mesh = results['mesh'].reshape(12, -1)
    rec = dict(tool='ocean_points_time', device=ctx.device_name(), source=list(oc['latitude'].shape), source_points=cloud.nsrc,
               cells=[cloud.ncx, cloud.ncy], target=[nlat, nlon], months=12, reps=args.reps,
               land_targets=int((land > 0.7).sum()),
               same_bits_rowmajor=bool(np.array_equal(results['rowmajor'].reshape(12, -1).view(np.uint64), mesh.view(np.uint64))),
               same_bits_permuted=bool(np.array_equal(results['permuted'].view(np.uint64),
                                                      np.ascontiguousarray(mesh[:, perm]).view(np.uint64))))
    for k, v in runs.items():
        for key in v[0]:
            vals = [r[key] for r in v]
            rec['%s_%s' % (k, key)] = round(float(np.median(vals)), 4)
            rec['%s_%s_minmax' % (k, key)] = [round(min(vals), 4), round(max(vals), 4)]
    for k in ('rowmajor', 'permuted'):
        rec['%s_gather_over_mesh_kernel' % k] = round(rec['%s_gather_ms' % k] / rec['mesh_kernel_ms'], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
