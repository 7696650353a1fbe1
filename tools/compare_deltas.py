#!/usr/bin/env python
"""Compare two directories of step_03 `--debug_mode` output (interpolate_time or interpolate_full), file by file.

    python tools/compare_deltas.py DIR_A DIR_B [--atol A] [--rtol R]

For every NetCDF-3 file name present in both directories the variable the file is named after is compared: the two
dtypes, max |a - b| and max |a - b| / |b| over the points where both are finite, and whether the NaN masks agree.  One
JSON line ends the report.  Exit status 1 when a file exceeds `--atol + --rtol * |b|` somewhere, differs in shape or NaN
mask, or when no file name is common to both directories; files present in one directory only are listed.

CPU only.  Output of the reference written as NetCDF-4 goes through `nccopy -k classic in.nc out.nc` first
(INTEGRATION.md)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402


def data_variable(ds):
    """The one variable of a delta file that is not a coordinate variable (most dimensions wins)."""
    best = None
    for name, f in ds.variables.items():
        if f.dims == (name,):
            continue
        if best is None or len(f.dims) > len(ds[best].dims):
            best = name
    return best


def compare_arrays(a, b, atol, rtol):
    a, b = np.asarray(a), np.asarray(b)
    rec = dict(dtype_a=str(a.dtype), dtype_b=str(b.dtype), shape_a=list(a.shape), shape_b=list(b.shape))
    if a.shape != b.shape:
        rec.update(ok=False, why='shape')
        return rec
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    fin = np.isfinite(a64) & np.isfinite(b64)
    rec['nan_mask_equal'] = bool(np.array_equal(np.isnan(a64), np.isnan(b64)))
    rec['nan_a'], rec['nan_b'] = int(np.isnan(a64).sum()), int(np.isnan(b64).sum())
    d = np.abs(a64[fin] - b64[fin])
    ref = np.abs(b64[fin])
    rec['max_abs'] = float(d.max()) if d.size else 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(d == 0, 0.0, d / ref)
    rec['max_rel'] = float(rel.max()) if d.size else 0.0
    within = bool(np.all(d <= atol + rtol * ref))
    rec['ok'] = within and rec['nan_mask_equal'] and bool(np.array_equal(np.isfinite(a64), np.isfinite(b64)))
    if not rec['ok']:
        rec['why'] = 'values' if not within else 'nan mask'
    return rec


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('dir_a')
    p.add_argument('dir_b')
    p.add_argument('--atol', type=float, default=0.0)
    p.add_argument('--rtol', type=float, default=0.0)
    a = p.parse_args(argv)
    from pgw4era5_amd import ncio
    names_a = {f for f in os.listdir(a.dir_a) if f.endswith('.nc')}
    names_b = {f for f in os.listdir(a.dir_b) if f.endswith('.nc')}
    common = sorted(names_a & names_b)
    files, failed = {}, []
    for name in common:
        da = ncio.open_dataset(os.path.join(a.dir_a, name), decode_times=False)
        db = ncio.open_dataset(os.path.join(a.dir_b, name), decode_times=False)
        va, vb = data_variable(da), data_variable(db)
        if va is None or va != vb:
            rec = dict(ok=False, why='variable', variable_a=va, variable_b=vb)
        else:
            rec = dict(variable=va, **compare_arrays(da[va].values, db[vb].values, a.atol, a.rtol))
        files[name] = rec
        if rec['ok']:
            print('%-48s %s %s / %s  max|a-b| = %.3e  max rel = %.3e  NaN masks equal' %
                  (name, rec['variable'], rec['dtype_a'], rec['dtype_b'], rec['max_abs'], rec['max_rel']))
        else:
            failed.append(name)
            print('%-48s DIFFERS (%s): %s' % (name, rec['why'], json.dumps({k: v for k, v in rec.items() if k not in ('ok', 'why')})))
    only_a, only_b = sorted(names_a - names_b), sorted(names_b - names_a)
    for tag, names in (('only in ' + a.dir_a, only_a), ('only in ' + a.dir_b, only_b)):
        for n in names:
            print('%-48s %s' % (n, tag))
    ok = bool(common) and not failed
    print(json.dumps(dict(ok=ok, compared=len(common), failed=failed, only_a=only_a, only_b=only_b, atol=a.atol, rtol=a.rtol,
                          files=files)))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
