#!/usr/bin/env python
"""Time of k_delta_fields (pgw_delta_fields: the four interpolated deltas of step_03 --debug_mode interpolate_full in one
launch) at 1440 x 721 columns, L137, plev19 monthly records, float64 - beside the composed form the library already had:
the time interpolations (pgw_time_lerp of ta, hur, ua, va, tas, hurs, ps_hist) and four pgw_vert_interp_delta calls on the
interpolated records.

Both forms alternate IN THE SAME PROCESS after a warm-up run, --runs runs each; kernel times from pgw_profile_get (device
events around the launches).  Algorithmic bytes of the fused kernel: the four float64 outputs (4 * nlev * ncol * 8) plus the
gathered records (2 records * 4 variables * nplev * ncol * s) and the 2-D inputs; the composed form also writes and re-reads
the interpolated records.  The two forms must agree bit for bit (checked on the last run).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402

PEAK_TBS = 8.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--nlat', type=int, default=721)
    p.add_argument('--nlon', type=int, default=1440)
    p.add_argument('--nlev', type=int, default=137)
    p.add_argument('--runs', type=int, default=7)
    p.add_argument('--dtype', type=str, default='float64', choices=['float64', 'float32'])
    a = p.parse_args()
    from pgw4era5_amd import _lib, synthetic
    from pgw4era5_amd.device import default_context, dtype_tag
    ctx = default_context()
    lib, h = ctx.lib, ctx.handle
    dt = np.dtype(a.dtype)
    tag, s = dtype_tag(dt), dt.itemsize
    nlat, nlon, N = a.nlat, a.nlon, a.nlev
    ncol = nlat * nlon
    plev = np.ascontiguousarray(synthetic.PLEV19)
    S = len(plev)
    rng = np.random.default_rng(0)
    ak, bk = synthetic.hybrid_coefficients(N)
    ctx.set_levels(ak, bk)
    orog = 5000.0 * synthetic._smooth2d(rng, nlat, nlon) ** 3
    ps = 101325.0 * np.exp(-orog / 8000.0)
    pat = synthetic._smooth2d(rng, nlat, nlon)
    d_ps = ctx.to_device(ps[None].astype(dt), dt)
    x_hi, x_new = 31.0 * 86400e9, 17.625 * 86400e9                     # between two monthly records

    def rec3(scale):                                                   # two records (before, after) of a level variable
        prof = scale * (1.0 + np.cos(np.linspace(0, np.pi, S)))[:, None, None]
        return [ctx.to_device((prof * (0.8 + 0.4 * pat)[None] * f).astype(dt), dt) for f in (1.0, 1.1)]

    def rec2(field):
        return [ctx.to_device((field * f).astype(dt), dt) for f in (1.0, 1.0005)]

    R3 = {v: rec3(sc) for v, sc in (('ta', 2.0), ('hur', -3.0), ('ua', 1.0), ('va', -1.0))}
    R2 = dict(tas=rec2(2.0 * (0.8 + 0.4 * pat)), hurs=rec2(-2.0 * (2 * pat - 1)), ps_hist=rec2(ps * (1 + 0.002 * (2 * pat - 1))))
    out = {v: ctx.empty((1, N, nlat, nlon), np.float64) for v in R3}
    lerped = {v: ctx.empty(r[0].shape, dt) for v, r in list(R3.items()) + list(R2.items())}
    comp = {v: ctx.empty((1, N, nlat, nlon), dt) for v in R3}
    plev_p = plev.ctypes.data_as(_lib._dp)

    def fused():
        recs = [x.ptr for v in ('ta', 'hur', 'ua', 'va') for x in R3[v]] + [x.ptr for v in ('tas', 'hurs', 'ps_hist') for x in R2[v]]
        ctx._check(lib.pgw_delta_fields(h, tag, 0, 1, N, S, ncol, plev_p, d_ps.ptr, *recs, x_hi, x_new, 1,
                                        *[out[v].ptr for v in ('ta', 'hur', 'ua', 'va')]))

    def composed():
        for v, r in list(R3.items()) + list(R2.items()):
            ctx._check(lib.pgw_time_lerp(h, tag, r[0].size, r[0].ptr, r[1].ptr, x_hi, x_new, lerped[v].ptr))
        for v in R3:
            sfc = [None] * 4
            if v in ('ta', 'hur'):
                sfc = [lerped[v + 's'].ptr, None, lerped['ps_hist'].ptr, None]
            ctx._check(lib.pgw_vert_interp_delta(h, tag, 1, S, N, ncol, plev_p, lerped[v].ptr, None, 0.0, 0.0, *sfc, None, d_ps.ptr, 1,
                                                 None, comp[v].ptr))

    ctx.profile(True)

    def timed(fn, kids):
        ctx.profile_reset()
        fn()
        ctx.sync()
        return [ctx.profile_get(k)[1] for k in kids]

    t = dict(fused=[], composed=[], composed_lerp=[], composed_interp=[])
    for i in range(a.runs + 1):                                       # run 0 warms up
        t['fused'].append(timed(fused, ['delta_fields'])[0])
        lerp_ms, interp_ms = timed(composed, ['time_lerp', 'vert_interp_delta'])
        t['composed_lerp'].append(lerp_ms)
        t['composed_interp'].append(interp_ms)
        t['composed'].append(lerp_ms + interp_ms)
    ctx.profile(False)
    same = all(np.array_equal(out[v].numpy(), comp[v].numpy().astype(np.float64)) for v in R3) if dt == np.dtype('float64') else None
    out_bytes = 4 * N * ncol * 8
    gather_bytes = 2 * 4 * S * ncol * s + (2 * 3 + 1) * ncol * s
    res = dict(device=ctx.device_name(), nlat=nlat, nlon=nlon, nlev=N, nplev=S, dtype=a.dtype, runs=a.runs,
               bytes=dict(outputs=out_bytes, records_and_2d=gather_bytes), fused_equals_composed=same)
    for key in t:
        ms = t[key][1:]
        res[key] = dict(ms=[round(m, 4) for m in ms], median_ms=round(statistics.median(ms), 4))
    med = res['fused']['median_ms']
    res['fused']['TB_per_s_outputs'] = round(out_bytes / med / 1e9, 3)
    res['fused']['TB_per_s_all'] = round((out_bytes + gather_bytes) / med / 1e9, 3)
    res['fused']['share_of_peak_all'] = round((out_bytes + gather_bytes) / med / 1e9 / PEAK_TBS, 3)
    res['composed_over_fused'] = round(res['composed']['median_ms'] / med, 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
