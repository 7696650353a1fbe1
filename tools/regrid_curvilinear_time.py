#!/usr/bin/env python
"""Timing of the curvilinear regridding (settings.i_use_xesmf_regridding = 1) at production size: a 192 x 384 global grid
handed over as 2-D coordinates -> 721 x 1440, 19 levels x 12 months = 228 planes.  Three things, device events
(pgw_profile_get / pgw_timer), every leg warmed up and the legs alternating in one process:
  locate - host bucket build (host clock) and k_cell_locate;
  apply  - k_regrid_sparse (with its row means) beside k_regrid on the same grid and planes;
  write  - the bare write of the output (a device memset of its bytes), the floor of a write-dominated kernel.
The apply is timed in both of its forms: `sparse` (a block stages its source window in LDS where it fits - every block of
this grid pair does) and `sparse_direct` (every block gathers from memory).
Prints one JSON line per storage type; `--out FILE` appends them to FILE (profiles/regrid_curvilinear_<tag>.json).
`--small` runs a 24 x 48 -> 37 x 72, 6-plane rehearsal of the same code path."""
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


def median(xs):
    return float(np.median(np.asarray(xs)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args(argv)
    shape = dict(nlat_src=24, nlon_src=48, nlat=37, nlon=72, nplev=3, ntime=2) if args.small else \
        dict(nlat_src=192, nlon_src=384, nlat=721, nlon=1440, nplev=19, ntime=12)
    ctx = default_context()
    lines = []
    for dt in (np.float64, np.float32):
        g = synthetic.make_gcm_grid_case(seed=4, dtype=dt, **shape)
        slat2, slon2 = np.meshgrid(g['src_lat'], g['src_lon'], indexing='ij')
        periodic = F.periodic_lon_rule(slon2)
        nplanes = shape['nplev'] * shape['ntime']
        ntarg = shape['nlat'] * shape['nlon']
        out_bytes = nplanes * ntarg * np.dtype(dt).itemsize
        src = ctx.to_device(g['field'], dt)

        # ---- locate: host part (unit vectors, buckets) on the host clock, the kernel by device events
        t0 = time.perf_counter()
        X = F.unit_vectors(slat2, slon2)
        nb, bstart, bcells = F.curvilinear_buckets(X, periodic)
        host_s = time.perf_counter() - t0
        F._WEIGHTS_CACHE.clear()
        F.curvilinear_weights(slat2, slon2, g['targ_lat'], g['targ_lon'], periodic)          # warm-up
        ctx.profile(True)
        loc = []
        for _ in range(3):
            F._WEIGHTS_CACHE.clear()
            ctx.profile_reset()
            wts = F.curvilinear_weights(slat2, slon2, g['targ_lat'], g['targ_lon'], periodic)
            loc.append(ctx.profile_get('cell_locate')[1])

        # ---- apply beside k_regrid beside the bare write, alternating
        def leg_sparse(direct):
            old = ctx.set_option('sparse_direct', direct)
            ctx.profile_reset()
            F.regrid_curvilinear(src, wts).free()
            ctx.set_option('sparse_direct', old)
            return ctx.profile_get('regrid_sparse')[1]

        def leg_regrid():
            ctx.profile_reset()
            F.regrid_field(src, g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon']).free()
            return ctx.profile_get('regrid')[1]

        scratch = ctx.empty((nplanes, shape['nlat'], shape['nlon']), dt)

        def leg_write():
            ctx.sync()
            ctx.timer_start()
            ctx._check(ctx.lib.pgw_memset(ctx.handle, scratch.ptr, 0, scratch.nbytes))
            return ctx.timer_stop()

        legs = dict(sparse=lambda: leg_sparse(0), sparse_direct=lambda: leg_sparse(1), regrid=leg_regrid, write=leg_write)
        for f in legs.values():
            f()                                                          # warm-up of every leg
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
        ctx.profile(False)
        one = g['field'][0]                                              # the planes of one month: what the two schemes differ by
        diff = np.abs(F.regrid_curvilinear(one, wts).astype(np.float64)
                      - F.regrid_field(one, g['src_lat'], g['src_lon'], g['targ_lat'], g['targ_lon']).astype(np.float64))
        rec = dict(tool='regrid_curvilinear_time', device=ctx.device_name(), dtype=np.dtype(dt).name, shape=shape, planes=nplanes,
                   targets=ntarg, out_GB=round(out_bytes / 1e9, 3), buckets_nb=nb, bucket_entries=int(len(bcells)),
                   unmapped=wts.n_unmapped, locate_host_s=round(host_s, 3), locate_kernel_ms=round(median(loc), 3),
                   max_abs_diff_vs_regrid_field=float(np.nanmax(diff)))
        for k, v in ms.items():
            rec['%s_ms' % k] = round(median(v), 4)
            rec['%s_ms_minmax' % k] = [round(min(v), 4), round(max(v), 4)]
            rec['%s_out_GBps' % k] = round(out_bytes / 1e9 / (median(v) / 1e3), 1)
        print(json.dumps(rec))
        lines.append(json.dumps(rec))
        src.free(); scratch.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
