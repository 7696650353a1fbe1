#!/usr/bin/env python
"""Time of the hydrostatic check's kernel k_geopot_plev (pgw_geopot_on_plev) at 1440 x 721 columns, L137, plev19: the
two-state launch - both forms, `one_walk` (both states level by level in one loop) and `two_walks` (state a, then state b, in
the same launch) - beside the composed form (two one-state launches plus pgw_field_sub) and beside the bare read of the same
four level arrays (pgw_test_read_records, the access pattern of a column walk with no arithmetic).  Also the launches with the zg
record pair (phi_error, both forms) and the one-state launch.

All forms alternate IN THE SAME PROCESS after a warm-up run, --runs runs each (at least 7); kernel times from pgw_profile_get
(device events around the launches); medians are reported.  Algorithmic bytes of the two-state form: (4 N + 3) ncol s read,
S ncol 8 written.  The fused and composed results must be equal bit for bit (checked on the last run).  Prints one JSON line."""
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
    if a.runs < 7:
        p.error('--runs must be at least 7')
    from pgw4era5_amd import _lib, synthetic
    from pgw4era5_amd.constants import CON_G
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
    akm, bkm = 0.5 * (ak[1:] + ak[:-1]), 0.5 * (bk[1:] + bk[:-1])
    ctx.set_levels(ak, bk)
    orog = 5000.0 * synthetic._smooth2d(rng, nlat, nlon) ** 3
    ps = 101325.0 * np.exp(-orog / 8000.0)
    pat = synthetic._smooth2d(rng, nlat, nlon)
    ps_b = ps + 150.0 * (0.5 + pat)
    T = np.empty((1, N, nlat, nlon), dtype=dt)
    d = {}
    for name, p_s, warm in (('a', ps, 0.0), ('b', ps_b, 2.0)):         # level by level: no full-size float64 temporaries
        for l in range(N):
            T[0, l] = np.maximum(288.0 + 52.0 * np.log((akm[l] + p_s * bkm[l]) / 101325.0), 215.0) + warm * (0.8 + 0.4 * pat)
        d['T_' + name] = ctx.to_device(T, dt)
        for l in range(N):
            T[0, l] = 0.008 * np.clip((akm[l] + p_s * bkm[l]) / 101325.0, 0.0, 1.0) ** 3 * (0.2 + 0.8 * pat)
        d['QV_' + name] = ctx.to_device(T, dt)
        d['PS_' + name] = ctx.to_device(p_s[None].astype(dt), dt)
    del T
    d['FIS'] = ctx.to_device((9.80665 * orog)[None].astype(dt), dt)
    prof = (20.0 + 100.0 * np.clip(np.log(1e5 / plev) / np.log(1e3), 0, 1) ** 0.7)[:, None, None]
    zg = [ctx.to_device((prof * (0.9 + 0.2 * pat)[None] * f)[None].astype(dt), dt) for f in (1.0, 1.1)]
    x_hi, x_new = 31.0 * 86400e9, 17.625 * 86400e9                     # between two monthly records
    shp = (1, S, nlat, nlon)
    out = {k: ctx.empty(shp, np.float64) for k in ('one_walk', 'two_walks', 'error', 'phi_a', 'phi_b', 'composed')}
    plev_p = plev.ctypes.data_as(_lib._dp)

    def launch(o, two, form=0, err=False):
        b = [d['PS_b'].ptr, d['T_b'].ptr, d['QV_b'].ptr] if two else [None, None, None]
        z = [tag, zg[0].ptr, zg[1].ptr, x_hi, x_new] if err else [0, None, None, 0.0, 0.0]
        ctx._check(lib.pgw_geopot_on_plev(h, tag, tag, tag if two else 0, 1, S, ncol, plev_p, d['FIS'].ptr, d['PS_a'].ptr, d['T_a'].ptr,
                                          d['QV_a'].ptr, *b, *z, CON_G, form, o.ptr, None))

    def composed():
        launch(out['phi_a'], False)
        ctx._check(lib.pgw_geopot_on_plev(h, tag, tag, 0, 1, S, ncol, plev_p, d['FIS'].ptr, d['PS_b'].ptr, d['T_b'].ptr, d['QV_b'].ptr,
                                          None, None, None, 0, None, None, 0.0, 0.0, CON_G, 0, out['phi_b'].ptr, None))
        ctx._check(lib.pgw_field_sub(h, _lib.PGW_F64, out['composed'].size, out['phi_b'].ptr, out['phi_a'].ptr, out['composed'].ptr))

    def read4():
        for k in ('T_a', 'QV_a', 'T_b', 'QV_b'):
            ctx._check(lib.pgw_test_read_records(h, tag, N, ncol, d[k].ptr))

    forms = dict(one_walk=(lambda: launch(out['one_walk'], True, 0), ['integ_geopot']),
                 two_walks=(lambda: launch(out['two_walks'], True, 1), ['integ_geopot']),
                 composed=(composed, ['integ_geopot', 'field_sub']),
                 read_four_level_arrays=(read4, ['clim_read']),
                 error_one_walk=(lambda: launch(out['error'], True, 0, True), ['integ_geopot']),
                 error_two_walks=(lambda: launch(out['error'], True, 1, True), ['integ_geopot']),
                 one_state=(lambda: launch(out['phi_a'], False), ['integ_geopot']))
    ctx.profile(True)
    t = {k: [] for k in forms}
    for i in range(a.runs + 1):                                        # run 0 warms up
        for k, (fn, kids) in forms.items():
            ctx.profile_reset()
            fn()
            ctx.sync()
            t[k].append(sum(ctx.profile_get(kid)[1] for kid in kids))
    ctx.profile(False)
    composed()
    want = out['composed'].numpy()

    def bits(x):                                                       # every NaN as one pattern
        return np.where(np.isnan(x), np.uint64(0x7ff8000000000000), x.view(np.uint64))

    same = {k: bool(np.array_equal(bits(out[k].numpy()), bits(want))) for k in ('one_walk', 'two_walks')}
    read_bytes = (4 * N + 3) * ncol * s
    write_bytes = S * ncol * 8
    res = dict(device=ctx.device_name(), nlat=nlat, nlon=nlon, nlev=N, nplev=S, dtype=a.dtype, runs=a.runs,
               bytes=dict(read=read_bytes, written=write_bytes), fused_equals_composed=same,
               nan_share=round(float(np.isnan(want).mean()), 4))
    for k in t:
        ms = t[k][1:]
        res[k] = dict(ms=[round(m, 4) for m in ms], median_ms=round(statistics.median(ms), 4))
    for k in ('one_walk', 'two_walks', 'error_one_walk', 'error_two_walks'):
        res[k]['TB_per_s'] = round((read_bytes + write_bytes) / res[k]['median_ms'] / 1e9, 3)
        res[k]['share_of_peak'] = round(res[k]['TB_per_s'] / PEAK_TBS, 3)
        res[k]['composed_over_this'] = round(res['composed']['median_ms'] / res[k]['median_ms'], 3)
        res[k]['this_over_read'] = round(res[k]['median_ms'] / res['read_four_level_arrays']['median_ms'], 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
