#!/usr/bin/env python
"""Time of the climatology kernel (pgw_clim_accumulate) on one day-of-year bin of a CFday variable of MPI-ESM1-2-HR after
interp_to_plev: 30 records (30 years) of 99 x 192 x 384 float32 = 876 MB, well past the 256 MiB Infinity Cache.

Two forms of the launch: `first` and `last` both set (the normal case: no accumulator in memory; algorithmic bytes
(nrec + 1) * inner * s) and a carried chunk (neither set: sum and cnt read and written back, nrec * inner * s + 2 * inner *
12).  Each alternates IN THE SAME PROCESS with a bare read of the same arrays (pgw_test_read_records: the same grid, the
same loads, no arithmetic and no store; nrec * inner * s), warmed up, --runs runs each; kernel times from pgw_profile_get
(device events around the launch).

--e2e-gbytes G (default 1; 0 = skip): one `climatology_files` run end to end - a synthetic monthly series of that size is
written to --tmp, then read, binned (ymonmean), accumulated and written; seconds and seconds per GB of input.  That figure
is set by reading the file (pread per record, byte swap and fill-value decoding on the host, pageable upload), not by the
kernel.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402

PEAK_TBS = 8.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--records', type=int, default=30)
    p.add_argument('--shape', type=str, default='99,192,384')
    p.add_argument('--runs', type=int, default=7)
    p.add_argument('--nan-share', type=float, default=0.05, help='share of missing values in the records')
    p.add_argument('--e2e-gbytes', type=float, default=1.0)
    p.add_argument('--tmp', type=str, default=None, help='directory for the end-to-end files (default: the system temporary directory)')
    a = p.parse_args()
    from pgw4era5_amd import ncio, step_01_extract_deltas as s1
    from pgw4era5_amd.device import default_context, dtype_tag
    ctx = default_context()
    shape = tuple(int(n) for n in a.shape.split(','))
    inner, nrec = int(np.prod(shape)), a.records
    dt = np.dtype('float32')
    s = dt.itemsize
    rng = np.random.default_rng(0)
    d_x = ctx.empty((nrec,) + shape, dt)
    for r in range(nrec):
        rec = rng.normal(250.0, 20.0, shape).astype(dt)
        rec[rng.random(shape) < a.nan_share] = np.nan
        d_x.slab(r).copy_from(rec)
    d_sum, d_cnt, d_mean = ctx.zeros(shape, np.float64), ctx.zeros(shape, np.int32), ctx.empty(shape, dt)
    res = dict(device=ctx.device_name(), records=nrec, shape=list(shape), dtype=str(dt), input_GB=round(nrec * inner * s / 1e9, 3),
               runs=a.runs, nan_share=a.nan_share, cases={})

    def bare():
        ctx._check(ctx.lib.pgw_test_read_records(ctx.handle, dtype_tag(dt), nrec, inner, d_x.ptr))

    forms = (('first_and_last', lambda: s1._launch_clim(ctx, d_x, True, True, None, None, d_mean, dt), (nrec + 1) * inner * s),
             ('carried_chunk', lambda: s1._launch_clim(ctx, d_x, False, False, d_sum, d_cnt, None, dt), nrec * inner * s + 2 * inner * 12))
    ctx.profile(True)

    def timed(fn, kid):
        ctx.profile_reset()
        fn()
        ctx.sync()
        return ctx.profile_get(kid)[1]

    for tag, fn, nbytes in forms:
        t = dict(kernel=[], bare_read=[])
        for i in range(a.runs + 1):                                   # run 0 warms up
            t['kernel'].append(timed(fn, 'clim_accumulate'))
            t['bare_read'].append(timed(bare, 'clim_read'))
        case = {}
        for key, b in (('kernel', nbytes), ('bare_read', nrec * inner * s)):
            ms = t[key][1:]
            med = statistics.median(ms)
            case[key] = dict(ms=[round(m, 4) for m in ms], median_ms=round(med, 4), bytes=b, TB_per_s=round(b / med / 1e9, 3),
                             share_of_peak=round(b / med / 1e9 / PEAK_TBS, 3))
        case['kernel_over_bare_read'] = round(case['kernel']['TB_per_s'] / case['bare_read']['TB_per_s'], 3)
        res['cases'][tag] = case
    ctx.profile(False)
    del d_x, d_sum, d_cnt, d_mean

    if a.e2e_gbytes > 0:
        years = max(1, int(round(a.e2e_gbytes * 1e9 / (12 * inner * s))))
        n = 12 * years
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            t_ax = (np.arange(n) * 30 + 15).astype(np.float64)
            data = rng.normal(250.0, 20.0, (n,) + shape).astype(dt)
            data[:, 0, :4, :4] = 1.0e20
            ds = ncio.Dataset(record_dim='time')
            ds['time'] = ncio.Field(t_ax, ('time',), {}, dict(units='days since 2000-01-01', calendar='360_day'))
            dims = ('time',) + tuple('d%d' % i for i in range(len(shape)))
            ds['ta'] = ncio.Field(data, dims, {}, dict(units='K', _FillValue=np.float32(1.0e20)))
            inp, out = os.path.join(tmp, 'ta_series.nc'), os.path.join(tmp, 'ta_clim.nc')
            ncio.to_netcdf(ds, inp)
            del ds, data
            t0 = time.perf_counter()
            s1.climatology_files(inp, out, 'ta', 'ymonmean')
            ctx.sync()
            sec = time.perf_counter() - t0
            gb = n * inner * s / 1e9
            res['end_to_end'] = dict(what='climatology_files ymonmean, file in the page cache: read, bin, upload, accumulate, write',
                                     records=n, input_GB=round(gb, 3), seconds=round(sec, 3), seconds_per_GB=round(sec / gb, 3))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
