#!/usr/bin/env python
"""Time of the delta check's kernel k_state_plev (pgw_state_on_plev: change + error of T, RH, U, V on the delta levels) at
721 x 1440 columns, L137, plev19, beside the composed entries that give the same numbers (2 x
pgw_specific_to_relative_humidity_hybrid, 8 x pgw_interp_hybrid_to_plev, 5 x pgw_time_lerp, pgw_field_sub) and beside the
bare read of the same level arrays (pgw_test_read_records: the access pattern of a column walk with no arithmetic).

The three alternate IN THE SAME PROCESS after a warm-up run, --runs runs each (at least 7); kernel times from
pgw_profile_get (device events around the launches); medians are reported.  Algorithmic bytes of the fused launch, from
the shapes: (8 N + 3) ncol s read (T, QV, U, V and PS per state, ps_hist), (8 S + 2) ncol s_delta of records read,
2 * 4 * S * ncol * 8 written.  The fused change must equal the composed one bit for bit, and the fused error the composed
change minus the interpolated record under the ps_hist mask (checked on the last run; with float32 storage against the
composed entries on copies widened on the host, which are not timed).  Writes one JSON line (also under profiles/)."""
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
    p.add_argument('--out', type=str, default=None, help='also write the JSON line here')
    a = p.parse_args()
    if a.runs < 7:
        p.error('--runs must be at least 7')
    from pgw4era5_amd import _lib, synthetic
    from pgw4era5_amd.device import default_context, dtype_tag
    import ctypes as C
    ctx = default_context()
    lib, h = ctx.lib, ctx.handle
    dt, f64 = np.dtype(a.dtype), np.dtype('float64')
    tag, s = dtype_tag(dt), dt.itemsize
    widen = dt != f64
    nlat, nlon, N = a.nlat, a.nlon, a.nlev
    ncol = nlat * nlon
    plev = np.ascontiguousarray(np.sort(synthetic.PLEV19))             # the composed entry takes an ascending list
    S = len(plev)
    rng = np.random.default_rng(0)
    ak, bk = synthetic.hybrid_coefficients(N)
    akm, bkm = np.ascontiguousarray(0.5 * (ak[1:] + ak[:-1])), np.ascontiguousarray(0.5 * (bk[1:] + bk[:-1]))
    ctx.set_levels(ak, bk)
    orog = 5000.0 * synthetic._smooth2d(rng, nlat, nlon) ** 3
    ps = 101325.0 * np.exp(-orog / 8000.0)
    pat = synthetic._smooth2d(rng, nlat, nlon)
    ps_b = ps + 150.0 * (0.5 + pat)
    X = np.empty((1, N, nlat, nlon), dtype=dt)
    d, w = {}, {}                                                      # storage dtype; widened copies for the check

    def put(name):
        d[name] = ctx.to_device(X, dt)
        if widen:
            w[name] = ctx.to_device(X.astype(f64), f64)

    for name, p_s, warm in (('a', ps, 0.0), ('b', ps_b, 2.0)):         # level by level: no full-size float64 temporaries
        for l in range(N):
            X[0, l] = np.maximum(288.0 + 52.0 * np.log((akm[l] + p_s * bkm[l]) / 101325.0), 215.0) + warm * (0.8 + 0.4 * pat)
        put('T_' + name)
        for l in range(N):
            X[0, l] = 0.008 * np.clip((akm[l] + p_s * bkm[l]) / 101325.0, 0.0, 1.0) ** 3 * (0.2 + 0.8 * pat)
        put('QV_' + name)
        for l in range(N):
            X[0, l] = (25.0 - 30.0 * (akm[l] + p_s * bkm[l]) / 101325.0) * (pat - 0.3) + warm
        put('U_' + name)
        for l in range(N):
            X[0, l] = 8.0 * (0.5 - pat) * (1.0 + l / N) - 0.5 * warm
        put('V_' + name)
        d['PS_' + name] = ctx.to_device(p_s[None].astype(dt), dt)
        if widen:
            w['PS_' + name] = ctx.to_device(p_s[None].astype(dt).astype(f64), f64)
    del X
    if not widen:
        w = d
    prof = (np.clip(np.log(1e5 / plev) / np.log(1e3), 0, 1) ** 0.7)[:, None, None]
    rec, wrec = {}, {}
    for i, v in enumerate(('ta', 'hur', 'ua', 'va')):
        for j, f in enumerate((1.0, 1.1)):
            r = ((2.0 + i) * (0.5 + prof) * (0.9 + 0.2 * pat)[None] * f)[None].astype(dt)
            rec[v, j] = ctx.to_device(r, dt)
            wrec[v, j] = ctx.to_device(r.astype(f64), f64) if widen else rec[v, j]
    for j, f in enumerate((1.0, 1.001)):
        r = (ps * f - 300.0)[None].astype(dt)
        rec['ps_hist', j] = ctx.to_device(r, dt)
        wrec['ps_hist', j] = ctx.to_device(r.astype(f64), f64) if widen else rec['ps_hist', j]
    names = ('ta', 'hur', 'ua', 'va', 'ps_hist')
    x_hi = (C.c_double * 5)(*[31.0 * 86400e9] * 5)
    x_new = (C.c_double * 5)(*[(17.625 + 0.5 * i) * 86400e9 for i in range(5)])        # every variable on its own axis
    shp = (4, 1, S, nlat, nlon)
    out = {k: ctx.empty(shp, f64) for k in ('change', 'error', 'x_a', 'x_b', 'composed')}
    rh = {k: ctx.empty((1, N, nlat, nlon), dt) for k in 'ab'}
    lerped = {v: ctx.empty((1, S, nlat, nlon) if v != 'ps_hist' else (1, nlat, nlon), dt) for v in names}
    plev_p, akm_p, bkm_p = (x.ctypes.data_as(_lib._dp) for x in (plev, akm, bkm))
    rb = C.cast((C.c_void_p * 4)(*[rec[v, 0].ptr for v in names[:4]]), _lib._vpp)
    ra = C.cast((C.c_void_p * 4)(*[rec[v, 1].ptr for v in names[:4]]), _lib._vpp)

    def fused():
        ctx._check(lib.pgw_state_on_plev(h, tag, tag, tag, 1, S, ncol, plev_p, *[d[k + '_a'].ptr for k in ('PS', 'T', 'QV', 'U', 'V')],
                                         *[d[k + '_b'].ptr for k in ('PS', 'T', 'QV', 'U', 'V')], tag, rb, ra, rec['ps_hist', 0].ptr,
                                         rec['ps_hist', 1].ptr, x_hi, x_new, out['change'].ptr, out['error'].ptr))

    def composed(src=None, recs=None, t_in=None, rh_=None, lerp_=None):
        src, recs, t_in, rh_, lerp_ = src or d, recs or rec, tag if t_in is None else t_in, rh_ or rh, lerp_ or lerped
        for st in 'ab':
            ctx._check(lib.pgw_specific_to_relative_humidity_hybrid(h, t_in, 1, ncol, src['QV_' + st].ptr, src['PS_' + st].ptr,
                                                                    src['T_' + st].ptr, rh_[st].ptr))
            for i, x in enumerate((src['T_' + st], rh_[st], src['U_' + st], src['V_' + st])):
                ctx._check(lib.pgw_interp_hybrid_to_plev(h, t_in, _lib.PGW_F64, 1, N, S, ncol, x.ptr, src['PS_' + st].ptr, akm_p, bkm_p,
                                                         plev_p, _lib.EXTRAP['nan'], 0, 0, out['x_' + st].slab(i).ptr))
        for i, v in enumerate(names):
            ctx._check(lib.pgw_time_lerp(h, t_in, lerp_[v].size, recs[v, 0].ptr, recs[v, 1].ptr, x_hi[i], x_new[i], lerp_[v].ptr))
        ctx._check(lib.pgw_field_sub(h, _lib.PGW_F64, out['composed'].size, out['x_b'].ptr, out['x_a'].ptr, out['composed'].ptr))

    def read_levels():
        for st in 'ab':
            for k in ('T_', 'QV_', 'U_', 'V_'):
                ctx._check(lib.pgw_test_read_records(h, tag, N, ncol, d[k + st].ptr))

    forms = dict(fused=(fused, ['hybrid_to_plev']), composed=(composed, ['q_to_rh', 'hybrid_to_plev', 'time_lerp', 'field_sub']),
                 read_level_arrays=(read_levels, ['clim_read']))
    ctx.profile(True)
    t = {k: [] for k in forms}
    for i in range(a.runs + 1):                                        # run 0 warms up
        for k, (fn, kids) in forms.items():
            ctx.profile_reset()
            fn()
            ctx.sync()
            t[k].append(sum(ctx.profile_get(kid)[1] for kid in kids))
    ctx.profile(False)
    # the check: float64 arithmetic on the stored values, so float32 storage is composed on the widened copies
    if widen:
        rh64 = {k: ctx.empty((1, N, nlat, nlon), f64) for k in 'ab'}
        lerp64 = {v: ctx.empty(lerped[v].shape, f64) for v in names}
        composed(w, wrec, _lib.PGW_F64, rh64, lerp64)
    else:
        lerp64 = lerped
        composed()
    ctx.sync()

    def bits(x):                                                       # every NaN as one pattern
        return np.where(np.isnan(x), np.uint64(0x7ff8000000000000), x.view(np.uint64))

    want = out['composed'].numpy()
    change = out['change'].numpy()
    same_change = bool(np.array_equal(bits(change), bits(want)))
    error = out['error'].numpy()
    above = plev[None, :, None, None] < lerp64['ps_hist'].numpy()[:, None]
    same_error = True
    for i, v in enumerate(names[:4]):
        same_error = same_error and bool(np.array_equal(bits(error[i]), bits(np.where(above, want[i] - lerp64[v].numpy(), np.nan))))
    read_bytes = (8 * N + 3) * ncol * s + (8 * S + 2) * ncol * s
    write_bytes = 2 * 4 * S * ncol * 8
    res = dict(device=ctx.device_name(), nlat=nlat, nlon=nlon, nlev=N, nplev=S, dtype=a.dtype, runs=a.runs,
               bytes=dict(read_levels=(8 * N + 3) * ncol * s, read_records=(8 * S + 2) * ncol * s, written=write_bytes),
               fused_change_equals_composed=same_change, fused_error_equals_composed=same_error,
               nan_share=dict(change=round(float(np.isnan(change).mean()), 4), error=round(float(np.isnan(error).mean()), 4)))
    for k in t:
        ms = t[k][1:]
        res[k] = dict(ms=[round(m, 4) for m in ms], median_ms=round(statistics.median(ms), 4))
    f = res['fused']
    f['TB_per_s'] = round((read_bytes + write_bytes) / f['median_ms'] / 1e9, 3)
    f['share_of_peak'] = round(f['TB_per_s'] / PEAK_TBS, 3)
    f['composed_over_this'] = round(res['composed']['median_ms'] / f['median_ms'], 3)
    f['this_over_read'] = round(f['median_ms'] / res['read_level_arrays']['median_ms'], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
