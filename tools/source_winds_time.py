#!/usr/bin/env python
"""Timing of the winds' way from a rotated-pole SOURCE grid (`step_02 regridding --source_winds` with
settings.i_use_xesmf_regridding = 1): ua and va of a 412 x 424 EURO-CORDEX-like rotated grid, 12 x 19 planes, float32 and
float64, onto the 721 x 1440 mesh (`mesh`: source rotation only - most of the mesh lies outside the domain and is unmapped) and
onto a second rotated grid with another pole inside the domain (`rotated`: both rotations).  Three legs:
  fused     pgw_regrid_sparse_wind (k_row_mean_plain_wind, k_regrid_sparse_wind): one launch pair;
  composed  pgw_rotate_pair(inverse) on the sources, pgw_regrid_sparse on each component, pgw_rotate_pair on the outputs
            where the target is rotated: the definition, two more passes over the sources and up to two over the outputs;
  write     a device memset of the two outputs' bytes, the floor of a write-dominated kernel.
Device events (the `regrid` and `regrid_sparse` profile entries together; pgw_timer for the memset), every leg warmed up, the
legs alternating in one process, median and min-max of `--reps` (9, at least 5).  Before every timed leg an output-sized
scratch array is overwritten once, untimed, so that each leg meets the same cache state.  The weights are located once, outside
the events.  The legs' outputs are compared bit for bit before anything is timed (an AssertionError otherwise).
Prints one JSON line per case and storage type; `--out FILE` appends them to FILE.  `--small`: a 24 x 48 source, a 37 x 72
mesh, 20 x 22 rotated targets and 6 planes, a rehearsal of the tool."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                       # noqa: E402
from pgw4era5_amd import functions as F, synthetic                       # noqa: E402
from pgw4era5_amd.device import default_context                          # noqa: E402

SOURCE_POLE, TARGET_POLE = (39.25, -162.0), (43.0, -170.0)


def run(ctx, case, dt, slat, slon, ua, va, tlat, tlon, target_pole, reps):
    nplanes = int(np.prod(ua.shape[:-2]))
    wts = F.curvilinear_weights(slat, slon, tlat, tlon, False)
    ntarg = int(np.prod(wts.targ_shape))
    out_bytes = 2 * nplanes * ntarg * np.dtype(dt).itemsize
    d_u, d_v = ctx.to_device(ua, dt), ctx.to_device(va, dt)
    src = F.wind_rotation(ctx.to_device(slat), ctx.to_device(slon), *SOURCE_POLE)
    targ = (None, None)
    if target_pole is not None:
        targ = F.wind_rotation(ctx.to_device(tlat), ctx.to_device(tlon), *target_pole)

    def fused():
        return F.regrid_curvilinear_wind(d_u, d_v, wts, *src, *targ)

    def composed():
        ug, vg = F.rotate_wind(d_u, d_v, *src, inverse=True)
        ur, vr = F.regrid_curvilinear(ug, wts), F.regrid_curvilinear(vg, wts)
        ug.free(), vg.free()
        if target_pole is None:
            return ur, vr
        out = F.rotate_wind(ur, vr, *targ)
        ur.free(), vr.free()
        return out

    a, b = fused(), composed()                                           # warm-up of both, and the same bits
    same = True
    for x, y in zip(a, b):                                               # one component at a time: the host holds two copies
        same = same and np.array_equal(x.numpy().view(np.uint8), y.numpy().view(np.uint8))
        x.free(), y.free()
    assert same, '%s %s: the fused entry and the composed form differ' % (case, np.dtype(dt).name)
    scratch = ctx.empty((out_bytes,), np.uint8)

    def profiled(f):
        def leg():
            ctx.profile_reset()
            for x in f():
                x.free()
            return ctx.profile_get('regrid')[1] + ctx.profile_get('regrid_sparse')[1]
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
    rec = dict(tool='source_winds_time', case=case, device=ctx.device_name(), dtype=np.dtype(dt).name, source=list(slat.shape),
               target=list(wts.targ_shape), unmapped=wts.n_unmapped, planes=nplanes, out_GB=round(out_bytes / 1e9, 3), reps=reps,
               same_bits=bool(same))
    for k, v in ms.items():
        rec['%s_ms' % k] = round(float(np.median(v)), 4)
        rec['%s_ms_minmax' % k] = [round(min(v), 4), round(max(v), 4)]
        rec['%s_out_GBps' % k] = round(out_bytes / 1e9 / (float(np.median(v)) / 1e3), 1)
    rec['fused_over_composed'] = round(rec['fused_ms'] / rec['composed_ms'], 3)
    for x in (d_u, d_v, scratch) + tuple(src) + tuple(x for x in targ if x is not None):
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
    ny, nx, planes = (24, 48, (2, 3)) if args.small else (412, 424, (12, 19))
    _, _, slat, slon = synthetic.rotated_pole_grid(ny, nx)
    mesh = (np.linspace(90.0, -90.0, 37), np.arange(72) * 5.0) if args.small else (np.linspace(90.0, -90.0, 721), np.arange(1440) * 0.25)
    _, _, rlat, rlon = synthetic.rotated_pole_grid(*((20, 22) if args.small else (412, 424)), *TARGET_POLE, rlat_range=(-9.0, 9.0),
                                                   rlon_range=(-9.0, 19.0))
    ctx = default_context()
    lines = []
    for dt in (np.float32, np.float64):
        rng = np.random.default_rng(4)
        ua, va = ((10.0 * rng.standard_normal(planes + (ny, nx))).astype(dt) for _ in range(2))
        lines.append(run(ctx, 'mesh', dt, slat, slon, ua, va, mesh[0], mesh[1], None, args.reps))
        lines.append(run(ctx, 'rotated', dt, slat, slon, ua, va, rlat, rlon, TARGET_POLE, args.reps))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
