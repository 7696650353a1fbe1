#!/usr/bin/env python
"""Time of the selection kernel (pgw_select_box) on a CFday variable of MPI-ESM1-2-HR after interp_to_plev: 30 records of
99 x 192 x 384 float32 (the shape of tools/clim_time.py, 876 MB).

Two cases: the reference's example box -73,37,-42,34 (`lonlat_box` on the model's 192 x 384 grid: 81 rows of 117 columns
from column 307, wrapping across 0 deg - an odd row length from an odd column, so one 4-byte word per lane) over all 99
levels, and separately a 27-of-34 level selection of whole 192 x 384 planes (the Emon bottom of Emon_add_top_from_Amon.sh;
16 bytes per lane) on 30 records of 34 levels.  Each alternates IN THE SAME PROCESS with `pgw_memcpy_d2d` of the same
number of output bytes, warmed up, --runs runs each; times from pgw_timer_start / pgw_timer_stop (device events around the
call).  Both move 2 x the output bytes (read + write); the kernel's reads are rows scattered over the source, the copy's are
one contiguous stretch.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402

PEAK_TBS = 8.0
EMON_BOTTOM = 27                                                       # of 34 levels: Emon_add_top_from_Amon.sh:45


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--records', type=int, default=30)
    p.add_argument('--shape', type=str, default='99,192,384')
    p.add_argument('--box', type=str, default='-73,37,-42,34')
    p.add_argument('--runs', type=int, default=9)
    a = p.parse_args()
    from pgw4era5_amd import step_01_extract_deltas as s1
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    nlev, nlat, nlon = (int(n) for n in a.shape.split(','))
    nrec, dt = a.records, np.dtype('float32')
    lat, lon = np.linspace(89.3, -89.3, nlat), np.arange(nlon) * (360.0 / nlon)
    lat0, nlat_sel, lon0, nlon_sel, _ = s1.lonlat_box(lat, lon, [float(b) for b in a.box.split(',')])
    rng = np.random.default_rng(0)
    plane = rng.normal(250.0, 20.0, (nlev, nlat, nlon)).astype(dt)
    res = dict(device=ctx.device_name(), records=nrec, shape=[nlev, nlat, nlon], dtype=str(dt), runs=a.runs, cases={})

    def measure(tag, src_shape, lev_idx, rows, cols, what):
        d_src = ctx.empty(src_shape, dt)
        for r in range(src_shape[0]):
            d_src.slab(r).copy_from(plane[:src_shape[1]])
        nsel = src_shape[1] if lev_idx is None else len(lev_idx)
        out_shape = (src_shape[0], nsel, rows[1], cols[1])
        d_out, d_copy = ctx.empty(out_shape, dt), ctx.empty(out_shape, dt)

        def kernel():
            s1._launch_select(ctx, dt.itemsize, src_shape[0], src_shape[1], nlat, nlon, d_src.ptr, lev_idx, rows, cols, nsel, 0, d_out.ptr)

        def d2d():
            ctx._check(ctx.lib.pgw_memcpy_d2d(ctx.handle, d_copy.ptr, d_out.ptr, d_out.nbytes))

        def timed(fn):
            ctx.timer_start()
            fn()
            return ctx.timer_stop()

        t = dict(kernel=[], d2d=[])
        for i in range(a.runs + 1):                                   # run 0 warms up
            t['kernel'].append(timed(kernel))
            t['d2d'].append(timed(d2d))
        moved = 2 * d_out.nbytes
        case = dict(what=what, source_GB=round(d_src.nbytes / 1e9, 3), output_GB=round(d_out.nbytes / 1e9, 3),
                    kept_share=round(d_out.nbytes / d_src.nbytes, 3), bytes_moved=moved)
        for key in ('kernel', 'd2d'):
            ms = t[key][1:]
            med = statistics.median(ms)
            case[key] = dict(ms=[round(m, 4) for m in ms], median_ms=round(med, 4), TB_per_s=round(moved / med / 1e9, 3),
                             share_of_peak=round(moved / med / 1e9 / PEAK_TBS, 3))
        case['kernel_over_d2d_time'] = round(case['kernel']['median_ms'] / case['d2d']['median_ms'], 3)
        res['cases'][tag] = case

    measure('box', (nrec, nlev, nlat, nlon), None, (lat0, nlat_sel), (lon0, nlon_sel),
            'box %s: rows %d..%d, %d columns from column %d (cyclic), all %d levels' % (a.box, lat0, lat0 + nlat_sel - 1, nlon_sel, lon0, nlev))
    nl = min(34, nlev)
    keep = np.arange(min(EMON_BOTTOM, nl), dtype=np.int32)
    measure('levels', (nrec, nl, nlat, nlon), keep, (0, nlat), (0, nlon), '%d of %d levels, whole planes' % (len(keep), nl))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
