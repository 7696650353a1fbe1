#!/usr/bin/env python
"""Kernel times of the function-level API under settings.function_dtype_flow = 'reference' beside 'common', on the operand
mixes a float32 ERA5 file produces, at 0.25 deg L137 (ncol = 721 x 1440 = 1,038,240, N = 137 model levels, S = 19 delta
levels), operands resident on the device:

  integ_geopot                   float64 pa_hl, float32 FIS / T / QV      (pgw_integ_geopot_mixed; V = 4 and V = 2)
  specific_to_relative_humidity  float32 QV, float64 pa, float32 T        (pgw_humidity_mixed)
  interp_logp_4d 'constant'      float32 T, float64 pa_era -> float64 pa_pgw   (pgw_interp_logp_4d_mixed)
  vert_interp_delta              float32 delta / tas / ps_hist, float64 target (pgw_vert_interp_delta_mixed)

against the way the same call is served under 'common': every operand a float64 copy, the uniform float64 kernels.  One
process, warmed up, the legs alternating, --runs runs each; times from pgw_profile_get (device events around the launch).
Algorithmic bytes per column are the operands read once plus the result written once.  Prints one JSON line; the condition
it reports per function: the 'reference' median is no slower than the 'common' median by more than the min-max spread of
the 'common' leg's own runs.  Host arrays additionally upload half the bytes for their float32 operands under 'reference'
(not timed here)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402

PEAK_TBS = 8.0
F32, F64 = 0, 1


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--nlat', type=int, default=721)
    p.add_argument('--nlon', type=int, default=1440)
    p.add_argument('--nlev', type=int, default=137)
    p.add_argument('--runs', type=int, default=5)
    a = p.parse_args()
    import ctypes as C
    from pgw4era5_amd import synthetic
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    lib, h = ctx.lib, ctx.handle
    nlat, nlon, N = a.nlat, a.nlon, a.nlev
    ncol = nlat * nlon
    tiny = synthetic.make_case(nlat=2, nlon=2, nlev=N, seed=0, dtype=np.float32)
    ak, bk = tiny['era']['ak'], tiny['era']['bk']
    akm, bkm = 0.5 * (ak[1:] - ak[:-1]) + ak[:-1], 0.5 * (bk[1:] - bk[:-1]) + bk[:-1]
    plev = np.ascontiguousarray(tiny['plev'], dtype=np.float64)
    S = len(plev)
    rng = np.random.default_rng(0)
    y, x = np.meshgrid(np.linspace(0, 1, nlat), np.linspace(0, 1, nlon), indexing='ij')
    ps = (1.0e5 - 4.0e4 * np.exp(-((x - 0.3)**2 + (y - 0.5)**2) / 0.02) + 2.0e3 * np.sin(9 * x) * np.cos(7 * y)).astype(np.float32)[None]
    e = lambda c: np.asarray(c)[None, :, None, None]
    pa_hl = e(ak) + ps[:, None] * e(bk)
    pa = e(akm) + ps[:, None] * e(bkm)
    pa2 = e(akm) + (ps + np.float32(350.0))[:, None] * e(bkm)
    eta = (pa / 1.0e5).astype(np.float32)
    T = (205.0 + 85.0 * eta + rng.standard_normal(pa.shape, dtype=np.float32)).astype(np.float32)
    QV = (1.2e-2 * eta**3 + 1e-6).astype(np.float32)
    FIS = ((1.0e5 - ps) * 0.8).astype(np.float32)
    delta = (2.0 + rng.standard_normal((1, S, nlat, nlon), dtype=np.float32)).astype(np.float32)
    tas = (2.5 + 0.1 * rng.standard_normal((1, nlat, nlon), dtype=np.float32)).astype(np.float32)
    psh = (ps * np.float32(0.999)).astype(np.float32)
    del eta
    up = lambda arr, dt: ctx.to_device(np.ascontiguousarray(arr, dtype=dt), np.dtype(dt))
    f4, f8 = np.float32, np.float64
    res = dict(device=ctx.device_name(), ncol=ncol, N=N, S=S, runs=a.runs, peak_TB_per_s=PEAK_TBS, cases={})

    def measure(name, kid, legs, bytes_per_col):
        """legs: {leg: callable}; alternating, run 0 warms up."""
        t = {k: [] for k in legs}
        ctx.profile(True)
        for i in range(a.runs + 1):
            for k, fn in legs.items():
                ctx.profile_reset()
                fn()
                ctx.sync()
                t[k].append(ctx.profile_get(kid)[1])
        ctx.profile(False)
        case = {}
        for k in legs:
            ms = t[k][1:]
            med = statistics.median(ms)
            b = bytes_per_col[k]
            case[k] = dict(ms=[round(m, 4) for m in ms], median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                           bytes_per_column=b, TB_per_s=round(ncol * b / med / 1e9, 3), share_of_peak=round(ncol * b / med / 1e9 / PEAK_TBS, 3))
        spread = case['common']['max_ms'] - case['common']['min_ms']
        for k in legs:
            if k != 'common':
                case[k]['no_slower_than_common_within_its_spread'] = bool(case[k]['median_ms'] <= case['common']['median_ms'] + spread)
        res['cases'][name] = case

    # ---- integ_geopot
    d_ph = up(pa_hl, f8)
    d_z4, d_t4, d_q4 = up(FIS, f4), up(T, f4), up(QV, f4)
    d_z8, d_t8, d_q8 = up(FIS, f8), up(T, f8), up(QV, f8)
    out2 = ctx.empty((1, nlat, nlon), f8)

    def geo_ref(vec):
        def f():
            ctx.set_option('mixed_vec', vec)
            ctx._check(lib.pgw_integ_geopot_mixed(h, F64, F32, F32, F32, 1, N, ncol, d_ph.ptr, d_z4.ptr, d_t4.ptr, d_q4.ptr, 30000.0, None, out2.ptr, 1))
        return f

    def geo_common():
        ctx._check(lib.pgw_integ_geopot(h, F64, 1, N, ncol, d_ph.ptr, d_z8.ptr, d_t8.ptr, d_q8.ptr, 30000.0, None, out2.ptr, 1))
    measure('integ_geopot', 'integ_geopot', {'reference_v4': geo_ref(4), 'reference_v2': geo_ref(2), 'common': geo_common},
            {'reference_v4': 16 * N + 8 + 4 + 8, 'reference_v2': 16 * N + 8 + 4 + 8, 'common': 24 * N + 8 + 8 + 8})
    ctx.set_option('mixed_vec', 4)
    del d_ph, d_z4, d_z8

    # ---- specific_to_relative_humidity
    d_pa = up(pa, f8)
    out4 = ctx.empty(pa.shape, f8)
    n = int(pa.size)
    measure('specific_to_relative_humidity', 'q_to_rh',
            {'reference': lambda: ctx._check(lib.pgw_humidity_mixed(h, 5, F32, F64, F32, n, d_q4.ptr, d_pa.ptr, d_t4.ptr, out4.ptr)),
             'common': lambda: ctx._check(lib.pgw_specific_to_relative_humidity(h, F64, n, d_q8.ptr, d_pa.ptr, d_t8.ptr, out4.ptr))},
            {'reference': 24 * N, 'common': 32 * N})
    del d_q4, d_q8

    # ---- interp_logp_4d, 'constant': T from the ERA levels to the levels of another surface pressure
    d_pa2 = up(pa2, f8)
    measure('interp_logp_4d', 'interp_logp',
            {'reference': lambda: ctx._check(lib.pgw_interp_logp_4d_mixed(h, F32, F64, 1, N, N, ncol, d_t4.ptr, d_pa.ptr, d_pa2.ptr, 2, 0, out4.ptr)),
             'common': lambda: ctx._check(lib.pgw_interp_logp_4d(h, F64, 1, N, N, ncol, d_t8.ptr, d_pa.ptr, d_pa2.ptr, 2, 0, out4.ptr))},
            {'reference': 28 * N, 'common': 32 * N})
    del d_pa2, d_t4, d_t8

    # ---- vert_interp_delta with the surface delta inserted
    dp = plev.ctypes.data_as(C.POINTER(C.c_double))
    d_d4, d_s4, d_h4 = up(delta, f4), up(tas, f4), up(psh, f4)
    d_d8, d_s8, d_h8 = up(delta, f8), up(tas, f8), up(psh, f8)
    measure('vert_interp_delta', 'vert_interp_delta',
            {'reference': lambda: ctx._check(lib.pgw_vert_interp_delta_mixed(h, F32, F32, F32, F64, F64, 1, S, N, ncol, dp, d_d4.ptr, d_s4.ptr,
                                                                             d_h4.ptr, d_pa.ptr, 1, None, out4.ptr)),
             'common': lambda: ctx._check(lib.pgw_vert_interp_delta(h, F64, 1, S, N, ncol, dp, d_d8.ptr, None, 0.0, 0.0, d_s8.ptr, None,
                                                                    d_h8.ptr, None, d_pa.ptr, None, 1, None, out4.ptr))},
            {'reference': 4 * S + 8 + 16 * N, 'common': 8 * S + 16 + 16 * N})
    print(json.dumps(res))


if __name__ == '__main__':
    main()
