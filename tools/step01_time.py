#!/usr/bin/env python
"""Time of the fused model-level -> pressure-level kernel (pgw_interp_hybrid_to_plev) beside the composed call
(pgw_interp_logp_4d on the two 4-D pressure fields, already on the device) on the CFday shape of MPI-ESM1-2-HR:
S = 95 model levels, N = 99 target levels (tests/golden/CFday_target_p_MPI-ESM1-2-HR.dat), 192 x 384 columns, as many
daily records as give at least --gbytes of input (default 2 GB, well past the 256 MiB Infinity Cache).

Same process, warmed up, the two alternating, --runs runs each; kernel times from pgw_profile_get (device events around
the launch).  Algorithmic bytes per column: fused S * s_in + s_in + N * s_out; composed (S + S + N + N) * 8 (the
composed call takes everything in one dtype, float64 here because the source pressure is float64).  Prints one JSON line.

--random-ps: surface pressure white noise per column instead of a smooth field (neighbouring lanes then sit on
different source levels: the worst case for the per-column source loads)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402

PEAK_TBS = 8.0


def coefficients(S):
    k = np.arange(S)
    eta = 0.02 + 0.98 * (k / (S - 1.0))**1.5
    n_pure = S // 3
    eta_c = eta[n_pure - 1]
    b = np.where(k < n_pure, 0.0, (np.maximum(eta - eta_c, 0.0) / (1.0 - eta_c))**1.2)
    ap = (eta - b) * 1.0e5
    ap[-1], b[-1] = 0.0, 1.0
    return ap, b


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--gbytes', type=float, default=2.0)
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--random-ps', action='store_true')
    p.add_argument('--vec1', action='store_true', help='set the option force_vec1 (matters for a build with PGW_H2P_MAX_V = 2)')
    p.add_argument('--no-composed', action='store_true', help='fused kernel only (for a kernel-trace run)')
    a = p.parse_args()
    from pgw4era5_amd import step_01_extract_deltas as s1
    from pgw4era5_amd.device import DeviceArray, default_context
    from pgw4era5_amd.operands import check_extrapolate
    ctx = default_context()
    if a.vec1:
        ctx.set_option('force_vec1', 1)
    S, nlat, nlon = 95, 192, 384
    ncol = nlat * nlon
    targ = s1.load_target_plev(os.path.join(ROOT, 'tests', 'golden', 'CFday_target_p_MPI-ESM1-2-HR.dat'))
    N = len(targ)
    ap, b = coefficients(S)
    rng = np.random.default_rng(0)
    res = dict(device=ctx.device_name(), S=S, N=N, ncol=ncol, runs=a.runs, ps='random' if a.random_ps else 'smooth',
               force_vec1=bool(a.vec1), cases={})
    mode = check_extrapolate('constant')
    for tag, dt, odt in (('F32->F64', np.float32, np.float64), ('F64->F64', np.float64, np.float64)):
        s_in, s_out = np.dtype(dt).itemsize, np.dtype(odt).itemsize
        nrec = int(np.ceil(a.gbytes * 1e9 / (S * ncol * s_in)))
        base = 4                                                      # distinct records; the block repeats them
        y, x = np.meshgrid(np.linspace(0, 1, nlat), np.linspace(0, 1, nlon), indexing='ij')
        if a.random_ps:
            ps = rng.uniform(5.0e4, 1.05e5, (base, nlat, nlon))
        else:
            ps = np.stack([1.0e5 - 4.5e4 * np.exp(-((x - 0.3 - 0.1 * i)**2 + (y - 0.5)**2) / 0.02) + 2.0e3 * np.sin(9 * x + i) * np.cos(7 * y)
                           for i in range(base)])
        ps = ps.astype(dt)
        eta = (ap + b * 1.0e5) / 1.0e5
        var = (200.0 + 90.0 * eta[None, :, None, None] + rng.normal(0, 1.0, (base, S, nlat, nlon))).astype(dt)
        reps = (nrec + base - 1) // base
        nrec = reps * base
        d_var, d_ps = ctx.empty((nrec, S, nlat, nlon), dt), ctx.empty((nrec, nlat, nlon), dt)
        for r in range(reps):
            DeviceArray(ctx, var.shape, dt, ptr=d_var.ptr + r * var.nbytes, owner=d_var).copy_from(var)
            DeviceArray(ctx, ps.shape, dt, ptr=d_ps.ptr + r * ps.nbytes, owner=d_ps).copy_from(ps)
        d_out = ctx.empty((nrec, N, nlat, nlon), odt)

        def fused():
            s1._launch_hybrid(ctx, d_var, d_ps, ap, b, targ, mode, False, False, d_out)

        comp = None
        if not a.no_composed:                                         # the composed call's operands, float64, on the device
            c_var, c_sp = ctx.empty((nrec, S, nlat, nlon), np.float64), ctx.empty((nrec, S, nlat, nlon), np.float64)
            c_tp, c_out = ctx.empty((nrec, N, nlat, nlon), np.float64), ctx.empty((nrec, N, nlat, nlon), np.float64)
            sp = ap[None, :, None, None] + b[None, :, None, None] * ps[:, None]
            tp = np.ascontiguousarray(np.broadcast_to(targ[None, :, None, None], (base, N, nlat, nlon)))
            v64 = var.astype(np.float64)
            for r in range(reps):
                DeviceArray(ctx, v64.shape, np.float64, ptr=c_var.ptr + r * v64.nbytes, owner=c_var).copy_from(v64)
                DeviceArray(ctx, sp.shape, np.float64, ptr=c_sp.ptr + r * sp.nbytes, owner=c_sp).copy_from(sp)
                DeviceArray(ctx, tp.shape, np.float64, ptr=c_tp.ptr + r * tp.nbytes, owner=c_tp).copy_from(tp)

            def comp():
                ctx._check(ctx.lib.pgw_interp_logp_4d(ctx.handle, 1, nrec, S, N, ncol, c_var.ptr, c_sp.ptr, c_tp.ptr, mode, 0, c_out.ptr))

        ctx.profile(True)
        t = dict(fused=[], composed=[])

        def timed(fn, kid, key):
            ctx.profile_reset()
            fn()
            ctx.sync()
            t[key].append(ctx.profile_get(kid)[1])

        for i in range(a.runs + 1):                                   # run 0 warms up
            timed(fused, 'hybrid_to_plev', 'fused')
            if comp:
                timed(comp, 'interp_logp', 'composed')
        ctx.profile(False)
        same = None
        if comp and dt == np.float64:                                 # the timed outputs, one record: the same bits
            g = DeviceArray(ctx, (1, N, nlat, nlon), np.float64, ptr=d_out.ptr, owner=d_out).numpy()
            w = DeviceArray(ctx, (1, N, nlat, nlon), np.float64, ptr=c_out.ptr, owner=c_out).numpy()
            same = bool(np.array_equal(g.view(np.uint64), w.view(np.uint64)))
        cols = nrec * ncol
        case = dict(records=nrec, input_GB=round(nrec * S * ncol * s_in / 1e9, 3), out_GB=round(nrec * N * ncol * s_out / 1e9, 3))
        for key, per_col in (('fused', S * s_in + s_in + N * s_out), ('composed', (2 * S + 2 * N) * 8)):
            if len(t[key]) > 1:
                ms = t[key][1:]
                med = statistics.median(ms)
                case[key] = dict(ms=[round(m, 3) for m in ms], median_ms=round(med, 3), bytes_per_column=per_col,
                                 TB_per_s=round(cols * per_col / med / 1e9, 3), share_of_peak=round(cols * per_col / med / 1e9 / PEAK_TBS, 3))
        if same is not None:
            case['fused_equals_composed_bits'] = same
        res['cases'][tag] = case
        del d_var, d_ps, d_out
        if comp:
            del c_var, c_sp, c_tp, c_out
    print(json.dumps(res))


if __name__ == '__main__':
    main()
