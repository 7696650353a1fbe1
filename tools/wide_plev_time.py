#!/usr/bin/env python
"""Per-file compute time of step_03 and time of k_delta_quad with the deltas on 19 pressure levels (the 64-entry plev table)
and on the reference's 99 CFday levels (the 128-entry table), in ONE process: synthetic 0.25 deg L137 file, float64 and
float32 reference-dtype mode, two delta records around the instant, zg on plev19 in both (fixed p_ref = 30000 Pa).

The two axes alternate after a warm-up file each, --runs files each; per-file time is the wall time of process_file_device
with reused outputs (the file plan) up to the stream's end, the kernel time from pgw_profile_get (device events).
Algorithmic bytes of the delta kernel: 4 ERA fields in, 4 PGW fields out, 2 records x S levels of 4 variables and 8 2-D
fields - bench.py's kernel_bytes('quad_delta').  The 99-level records add 4 variables x 2 records x 80 levels x ncol x
itemsize (a derivation from the shapes, not a measurement).  `bare`: the quad kernel's access pattern with no arithmetic on the
ERA inputs and the outputs of this run (Context.placement_probe); `share_of_bare` = algorithmic bytes / kernel time / that.
The 99-level result is checked against the 19-level one only for finiteness and the pass count.  Prints one JSON line; --out
also writes it to a file.

One GPU job:   timeout -k 10 500 python tools/wide_plev_time.py --out profiles/wide_plev_time.json"""
import argparse
import datetime as dt
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402

PLIST = os.path.join(ROOT, 'tests', 'golden', 'CFday_target_p_MPI-ESM1-2-HR.dat')
P_REF = 30000.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--nlat', type=int, default=721)
    p.add_argument('--nlon', type=int, default=1440)
    p.add_argument('--nlev', type=int, default=137)
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--modes', type=str, default='f64,f32ref')
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    from pgw4era5_amd import step_03_apply_to_era as s3, synthetic
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    nlat, nlon, N = a.nlat, a.nlon, a.nlev
    ncol = nlat * nlon
    plev99 = np.sort(np.loadtxt(PLIST))[::-1].copy()
    plev19 = np.ascontiguousarray(synthetic.PLEV19)
    nearest = np.argmin(np.abs(np.log(plev99)[:, None] - np.log(plev19)[None, :]), axis=1)
    stamp = dt.datetime(2006, 8, 2, 3)
    res = dict(device=ctx.device_name(), nlat=nlat, nlon=nlon, nlev=N, runs=a.runs, p_ref=P_REF, modes={})
    for mode in a.modes.split(','):
        dtype = np.dtype('float64' if mode == 'f64' else 'float32')
        ref = mode == 'f32ref'
        s, so = dtype.itemsize, (8 if ref else dtype.itemsize)
        case = synthetic.make_case(nlat=nlat, nlon=nlon, nlev=N, seed=1, dtype=dtype)
        times = case['delta_times'][6:8]                               # July and August: the two records around the instant
        d19 = {k: np.ascontiguousarray(v[6:8]) for k, v in case['deltas'].items()}
        era = s3._upload_era(ctx, case['era'], dtype)
        coeffs = dict(ak=case['era']['ak'], bk=case['era']['bk'], soil1=case['era']['soil1'])
        sets = {}
        sets[19] = s3.DeltaSet(ctx, d19, times, plev19, dtype, resident=True)
        d99 = dict(d19)
        for k in ('ta', 'hur', 'ua', 'va'):                            # each of the 99 levels takes the nearest plev19 record
            d99[k] = np.ascontiguousarray(d19[k][:, nearest])
        sets[99] = s3.DeltaSet(ctx, d99, times, plev99, dtype, resident=True)
        sets[99].plev_zg = plev19                                      # zg stays on its own axis
        del d99, case['deltas']
        outs = {19: {}, 99: {}}
        ctx.profile(True)
        t = {S: dict(file_ms=[], quad_ms=[], n_iter=None) for S in sets}
        for i in range(a.runs + 1):                                    # run 0 warms up (and draws the output buffers and the plan)
            for S in (19, 99):
                ctx.profile_reset()
                ctx.sync()
                t0 = time.perf_counter()
                out, info = s3.process_file_device(ctx, era, coeffs, sets[S], stamp, True, p_ref=P_REF, out=outs[S], ref_dtype=ref)
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3
                cnt, ms = ctx.profile_get('quad_delta')
                assert cnt == 1, cnt
                if i:
                    t[S]['file_ms'].append(wall)
                    t[S]['quad_ms'].append(ms)
                t[S]['n_iter'] = info['n_iter']
        ctx.profile(False)
        finite = {S: bool(np.isfinite(outs[S]['PS'].numpy()).all()) for S in sets}
        bare = ctx.placement_probe([era[k] for k in ('T', 'QV', 'U', 'V')], [outs[19][k] for k in ('T', 'QV', 'U', 'V')], reps=5)
        m = dict(dtype=dtype.name, ref_dtype=ref, bare_pattern_GBps=round(bare, 1),
                 extra_record_bytes_99_vs_19=4 * 2 * 80 * ncol * s)
        for S in sets:
            nbytes = (4 * N * s + 4 * N * so + (8 * S + 8) * s) * ncol
            q, f = statistics.median(t[S]['quad_ms']), statistics.median(t[S]['file_ms'])
            m['S%d' % S] = dict(n_iter=t[S]['n_iter'], ps_finite=finite[S],
                                file_ms=[round(x, 3) for x in t[S]['file_ms']], file_median_ms=round(f, 3),
                                quad_ms=[round(x, 4) for x in t[S]['quad_ms']], quad_median_ms=round(q, 4),
                                quad_algo_GB=round(nbytes / 1e9, 3), quad_GBps=round(nbytes / q / 1e6, 1),
                                share_of_bare=round(nbytes / q / 1e6 / bare, 3))
        m['quad_99_over_19'] = round(m['S99']['quad_median_ms'] / m['S19']['quad_median_ms'], 3)
        m['file_99_over_19'] = round(m['S99']['file_median_ms'] / m['S19']['file_median_ms'], 3)
        res['modes'][mode] = m
        for ds in sets.values():
            ds.free()
        ctx._file_plans.clear()                                        # (the plans point into the freed records)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
