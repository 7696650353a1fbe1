"""Cases of tests/test_source_deltas_hip.py and tests/test_source_deltas_host.py: step_03 on climate deltas that lie on the
GCM's grid (settings.delta_grid = 'source') and the regrid plan behind it (pgw_regrid_plan_create / _apply / _destroy).

Everything here is host code.  The reference of every comparison is the two-step route - `functions.regrid_field` /
`regrid_lat_lon` (pgw_regrid_bilinear) on the whole array, a cast on the host, and for the runs `step_02 regridding` into
files with step_03 on them - never the plan or the record provider themselves.  All comparisons are for equal bits, so no
tolerance is derived.  Each builder states the conditions its case exists for and `conditions()` asserts them on the CPU.
"""
import datetime as dt
import os

import numpy as np

WINDOW = 4                                   # DeltaSet.WINDOW: records of a variable kept on the device
GUARD = 4                                    # guard words in front of and behind an output slot
NFIELDS = (40, 3, 1)                         # applies on one plan, in this order: max_nfield first, then fewer planes
OFFSETS = (0, 1, 2)                          # elements between the 256-byte-aligned allocation + GUARD and the output slot


# ------------------------------------------------------------------ regrid plan: grid pairs
def _src(shape, descending, centred):
    nlat, nlon = shape
    if shape == (5, 8):
        lat = np.array([-72.0, -36.5, 0.0, 36.5, 72.0])
    else:
        lat = (-90.0 + 180.0 * (np.arange(nlat) + 0.5) / nlat) * (1 - 0.3 / nlat)
    lon = np.arange(nlon) * (360.0 / nlon) - (180.0 if centred else 0.0)
    return (lat[::-1].copy() if descending else lat), lon


TARGETS = {
    # both pole rows: rows at -90 and +90 and rows between the last source row and the pole; even row length (W = 2)
    'poles': (np.array([-90.0, -84.0, -40.5, 10.2, 77.7, 90.0]), np.array([0.0, 50.5, 133.0, 200.2, 310.0, 359.0])),
    # no pole row: max |lat| + dlat stays below 89.9 for both sources (dlat = 36 on the 5 x 8 source); even row length
    'no pole': (np.array([-50.0, -12.25, 0.0, 33.3, 50.0]), np.array([1.0, 44.0, 91.5, 182.0, 270.25, 358.0, 120.0, 15.0])),
    # a regional target, odd row length: W = 1 whatever the alignment
    'regional odd': (np.array([10.0, 17.5, 30.0, 45.0]), np.array([5.0, 11.0, 17.5, 22.0, 29.9, 33.0, 40.0])),
}


def grid_pairs():
    """(name, src_lat, src_lon, targ_lat, targ_lon): 5 x 8 and 48 x 96 sources, ascending / descending latitude, longitudes
    0 ... 360 / -180 ... 180, each with the three targets."""
    out = []
    for shape in ((5, 8), (48, 96)):
        for descending in (False, True):
            for centred in (False, True):
                lat, lon = _src(shape, descending, centred)
                for tname, (tlat, tlon) in TARGETS.items():
                    if descending and tname == 'poles':
                        # the reference takes dlat before it flips the rows (functions.py:779): it is negative here, no pole
                        # row is ever added and a target beyond the last row is the extent error (conditions())
                        continue
                    name = '%dx%d %s %s %s' % (shape[0], shape[1], 'desc' if descending else 'asc',
                                               '-180..180' if centred else '0..360', tname)
                    out.append((name, lat, lon, tlat, tlon))
    return out


def pair_ids():
    return [p[0] for p in grid_pairs()]


def plan_field(name, nfield, nlat_s, nlon_s, dtype, nan=None):
    """Planes about 100 apart (a plane taken from the wrong source plane shows).  nan = the pair's regrid_tables: NaN at three
    corners the targets interpolate between (their first, middle and last brackets), in the first plane; in the last plane
    the whole first and last source row (a NaN pole value where the target has pole rows).  Other planes stay finite."""
    rng = np.random.default_rng(abs(hash((len(name), nfield, nlat_s, nlon_s))) % (2 ** 31))
    f = rng.normal(size=(nfield, nlat_s, nlon_s)) * 7.0 + 100.0 * (1 + np.arange(nfield))[:, None, None]
    if nan is not None:
        rows = [int(r) for r in np.concatenate([nan['lat_lo'], nan['lat_hi']]) if 0 <= r < nlat_s]
        cols = [int(c) for c in np.concatenate([nan['lon_lo'], nan['lon_hi']])]
        for r, c in ((rows[0], cols[0]), (rows[len(rows) // 2], cols[len(cols) // 2]), (rows[-1], cols[-1])):
            f[0, r, c] = np.nan
        f[-1, 0, :] = np.nan
        f[-1, -1, :] = np.nan
    return f.astype(dtype)


# ------------------------------------------------------------------ records of a DeltaSet: time axes and walks
def monthly_axis():
    return np.array(['1996-%02d-15T12:00:00' % (m + 1) for m in range(12)], dtype='datetime64[s]')


def daily_axis_with_leap_day():
    """366 daily stamps of a leap year at 12:00: record 59 is Feb 29, which load_delta drops (functions.py:224-230)."""
    return (np.datetime64('1996-01-01T12:00:00', 's') + np.arange(366) * np.timedelta64(86400, 's')).astype('datetime64[s]')


def walk(axis_name):
    """Instants of one forward walk (years of the ERA5 files differ from the deltas': the stamps are re-yeared).  Monthly:
    from October into the next year's March, on a record now and then.  Daily: from Feb 26 over the dropped leap day, then
    Dec 29 over the year's end."""
    if axis_name == 'monthly':
        t, out = dt.datetime(2006, 10, 1, 0), []
        while t < dt.datetime(2007, 3, 20):
            out.append(t)
            t += dt.timedelta(days=9, hours=6)
        return out + [dt.datetime(2007, 4, 15, 12)]                    # exactly a record
    out = [dt.datetime(2007, 2, 26, 0) + dt.timedelta(hours=18 * i) for i in range(8)]
    out += [dt.datetime(2007, 12, 29, 6) + dt.timedelta(hours=18 * i) for i in range(8)]
    return out + [dt.datetime(2008, 1, 5, 12)]                         # exactly a record


def walk_brackets(times, instants):
    """[(record before, record after)] in FILE indices for every instant."""
    from pgw4era5_amd.step_03_apply_to_era import delta_time_bracket
    out = []
    for t in instants:
        ib, ia, _, _, keep = delta_time_bracket(times, t)
        out.append((int(keep[ib]), int(keep[ia])))
    return out


def revisit(times, instants):
    """An instant of the walk whose records were evicted by its end: the first one whose records are both absent from the
    last WINDOW distinct records used."""
    br = walk_brackets(times, instants)
    recent = []
    for b, a in br:
        for r in (b, a):
            if r in recent:
                recent.remove(r)
            recent.append(r)
    recent = recent[-WINDOW:]
    for t, (b, a) in zip(instants, br):
        if b not in recent and a not in recent:
            return t
    raise AssertionError('the walk evicts nothing')


def record_field(nrec, shape, dtype):
    """Records that all differ: record r is about r apart from its neighbours."""
    rng = np.random.default_rng(nrec)
    return (rng.normal(size=(nrec,) + shape) + np.arange(nrec).reshape((-1,) + (1,) * len(shape))).astype(dtype)


def conditions():
    """What the cases above exist for, asserted on the CPU (tests/test_source_deltas_host.py)."""
    from pgw4era5_amd import functions as F
    seen = set()
    for name, slat, slon, tlat, tlon in grid_pairs():
        tb = F.regrid_tables(slat, slon, tlat, tlon)
        poles = (tb['south_row'] >= 0, tb['north_row'] >= 0)
        if name.endswith('poles'):
            assert poles == (True, True) and len(tlon) % 2 == 0
            assert (tb['lat_lo'] == -1).any() and (tb['lat_hi'] == len(slat)).any()            # both pole rows are used
            assert tb['south_row'] == (len(slat) - 1 if slat[0] > slat[-1] else 0)
        elif name.endswith('no pole'):
            assert poles == (False, False) and len(tlon) % 2 == 0
        else:
            assert poles == (False, False) and len(tlon) % 2 == 1                               # W = 1
        assert not tb['lat_oob'].any() and not tb['lon_oob'].any()
        seen.add((len(slat), len(slon), bool(slat[0] > slat[-1]), bool(slon[0] < 0)))
    assert len(seen) == 8
    slat, slon = _src((5, 8), True, False)
    try:
        F.regrid_tables(slat, slon, *TARGETS['poles'])
        raise AssertionError('a descending source served a target at the poles')
    except ValueError as e:
        assert 'North or South' in str(e)
    assert max(NFIELDS) == NFIELDS[0] and set(NFIELDS) == {1, 3, 40}
    # the walks: more bracket moves than the window holds, across the year's end, over the dropped leap day
    for axis_name, times in (('monthly', monthly_axis()), ('daily', daily_axis_with_leap_day())):
        inst = walk(axis_name)
        br = walk_brackets(times, inst)
        assert all(a < b for a, b in zip(inst, inst[1:]))
        moves = sum(1 for p, q in zip(br, br[1:]) if p != q)
        assert moves > WINDOW, (axis_name, moves)
        assert any(b > a for b, a in br), axis_name                                             # before = last record, after = first
        assert any(b == a for b, a in br), axis_name                                            # an instant that is a record
        if axis_name == 'daily':
            assert len(times) == 366 and str(times[59])[5:10] == '02-29'
            assert all(59 not in p for p in br) and (58, 60) in br                              # Feb 28 -> Mar 1 brackets the gap
        t = revisit(times, inst)
        assert t in inst
    return True


# ------------------------------------------------------------------ step_03 runs: files
PLEV = np.array([100000.0, 92500.0, 85000.0, 70000.0, 60000.0, 50000.0, 40000.0, 30000.0, 25000.0, 20000.0, 15000.0, 10000.0,
                 7000.0, 5000.0, 3000.0, 2000.0, 1000.0, 500.0, 100.0])
LEVEL_VARS = ('ta', 'hur', 'ua', 'va', 'zg')
# instants of the runs: between two records, exactly on a record (the deltas' stamps are the 15th, 12:00), early January
# (before = December of the year before: the bracket wraps)
INSTANTS = (dt.datetime(2006, 7, 20, 6), dt.datetime(2006, 8, 15, 12), dt.datetime(2006, 1, 3, 0))


def rewrite(gcm_dir, dtype=None, fill=False, zg_levels=None, crop=None):
    """The files synthetic.write_gcm_files wrote, rewritten in place: every delta variable stored as `dtype`; crop = (lat0,
    lat1, lon0, lon1): the lat / lon variables cut to that box, a regional source that is not periodic; fill: the NaN of
    tos / siconc stored as `_FillValue` 1e20, a `_FillValue` nobody holds on ta and hur, ua packed as int16 with a
    scale_factor (decodes to float32), va packed as int16 with scale_factor and add_offset (decodes to float64);
    zg_levels: zg keeps only these indices of its plev axis (an axis of its own)."""
    from pgw4era5_amd import ncio
    for fname in sorted(os.listdir(gcm_dir)):
        var = fname.split('_')[0]
        path = os.path.join(gcm_dir, fname)
        ds = ncio.open_dataset(path)
        f = ds[var]
        vals, attrs = np.asarray(f.values), dict(f.attrs)
        if dtype is not None:
            vals = vals.astype(dtype)
        if crop is not None and 'lat' in f.dims:
            lat, lon = np.asarray(ds['lat'].values), np.asarray(ds['lon'].values)
            jj, ii = np.flatnonzero((lat >= crop[0]) & (lat <= crop[1])), np.flatnonzero((lon >= crop[2]) & (lon <= crop[3]))
            vals = np.ascontiguousarray(vals[..., jj[0]:jj[-1] + 1, ii[0]:ii[-1] + 1])
            ds['lat'] = ncio.Field(lat[jj], ('lat',), attrs=ds['lat'].attrs)
            ds['lon'] = ncio.Field(lon[ii], ('lon',), attrs=ds['lon'].attrs)
        if var == 'zg' and zg_levels is not None:
            vals = np.ascontiguousarray(vals[:, zg_levels])
            ds['plev'] = ncio.Field(np.asarray(ds['plev'].values)[zg_levels], ('plev',), attrs=ds['plev'].attrs)
        if fill:
            if var in ('tos', 'siconc'):
                vals = np.where(np.isnan(vals), vals.dtype.type(1e20), vals)
                attrs['_FillValue'] = vals.dtype.type(1e20)
            elif var in ('ta', 'hur'):
                attrs['_FillValue'] = vals.dtype.type(-9999.0)
            elif var in ('ua', 'va'):
                lo, hi = float(np.min(vals)), float(np.max(vals))
                scale = np.float64((hi - lo) / 60000.0)
                off = np.float64(0.5 * (hi + lo)) if var == 'va' else np.float64(0.0)
                if var == 'ua':
                    scale = np.float32(max(abs(lo), abs(hi)) / 30000.0)
                vals = np.rint((vals.astype(np.float64) - off) / np.float64(scale)).astype(np.int16)
                attrs['scale_factor'] = scale
                if var == 'va':
                    attrs['add_offset'] = off
        coords = {d: np.asarray(ds[d].values) for d in f.dims if d in ds}
        ds[var] = ncio.Field(vals, f.dims, coords, attrs)
        ncio.to_netcdf(ds, path)


def era_case(instant, dtype, seed=11, lat=None):
    """A synthetic ERA5 file at the size of BASELINE config 1 (10 x 10 columns, 20 levels), global: both pole rows; `lat`:
    other latitudes for its rows."""
    from pgw4era5_amd import synthetic
    c = synthetic.make_case(10, 10, 20, seed=seed, dtype=dtype, target_dt=instant)
    if lat is not None:
        c['lat'] = np.asarray(lat, dtype=np.float64)
    return c
