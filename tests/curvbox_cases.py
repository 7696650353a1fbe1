"""The lon-lat box on curvilinear grids (step_01 `curvilinear_box`, `pgw_box_mark_2d`): the numpy statement of the rule
and the grids, boxes and files the host and the GPU tests share.

`cdo` is not available, and its own index rule on curvilinear grids is not pinned: the statement
below IS the definition.  It is written here a second time, independently of the package (loops where the package uses
array expressions), so that a test compares two implementations."""
import numpy as np

REF_BOX = (-73.0, 37.0, -42.0, 34.0)          # the example box of extract_climate_delta.sh; straddles 0 deg
ASIA_BOX = (20.0, 120.0, -30.0, 60.0)
GLOBAL_BOX = (0.0, 360.0, -90.0, 90.0)
POLAR_BOX = (-180.0, 180.0, 60.0, 90.0)
BOXES = (REF_BOX, ASIA_BOX, GLOBAL_BOX, POLAR_BOX)
KERNEL_SHAPES = ((1, 1), (1, 64), (3, 1), (2, 63), (2, 65), (5, 130), (17, 257), (40, 60))
AUTO_SHAPES = ((40, 60), (30, 44), (12, 65), (8, 130), (17, 257), (9, 63))


# ------------------------------------------------------------------------------- the statement
def inside_ref(lat2d, lon2d, box):
    """inside[j, i]: float64 arithmetic on the exactly widened coordinates; both finite, min(lat1, lat2) <= lat <= max(lat1,
    lat2), lon + 360 k <= lon2 for the smallest integer k with lon + 360 k >= lon1 (the three lines of `lonlat_box`)."""
    lon1, lon2, lat1, lat2 = (float(b) for b in box)
    lat, lon = np.asarray(lat2d).astype(np.float64), np.asarray(lon2d).astype(np.float64)
    fin = np.isfinite(lat) & np.isfinite(lon)
    la, lo = np.where(fin, lat, 0.0), np.where(fin, lon, 0.0)
    k = np.ceil((lon1 - lo) / 360.0)
    k += (lo + 360.0 * k) < lon1
    k -= (lo + 360.0 * (k - 1.0)) >= lon1
    return fin & (la >= min(lat1, lat2)) & (la <= max(lat1, lat2)) & (lo + 360.0 * k <= lon2)


def flags_ref(lat2d, lon2d, box):
    """(row_any (nj) int32, col_any (ni) int32, n_inside)."""
    ins = inside_ref(lat2d, lon2d, box)
    return ins.any(axis=1).astype(np.int32), ins.any(axis=0).astype(np.int32), int(ins.sum())


def windows_ref(row_any, col_any, cyclic):
    """(j0, nj_sel, i0, ni_sel) by trying every start: rows first .. last flagged; columns first .. last flagged, or on a
    cyclic grid the complement of the longest cyclic run of unflagged columns, ties to the lowest start, all flagged ->
    (0, ni)."""
    rows = [j for j, f in enumerate(row_any) if f]
    cols = [bool(f) for f in col_any]
    ni = len(cols)
    assert rows and any(cols)
    j0, nj_sel = rows[0], rows[-1] - rows[0] + 1
    if not cyclic:
        on = [i for i, f in enumerate(cols) if f]
        return j0, nj_sel, on[0], on[-1] - on[0] + 1
    if all(cols):
        return j0, nj_sel, 0, ni
    best_len, best_start = 0, None
    for s in range(ni):                                            # ascending: the first longest run has the lowest start
        if cols[s] or not cols[(s - 1) % ni]:
            continue                                               # not the first column of an unflagged run
        n = 0
        while not cols[(s + n) % ni]:
            n += 1
        if n > best_len:
            best_len, best_start = n, s
    return j0, nj_sel, (best_start + best_len) % ni, ni - best_len


def _xyz(lat, lon):
    la, lo = np.deg2rad(lat), np.deg2rad(lon)
    return np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])


def cyclic_ref(lat2d, lon2d):
    """The 'auto' rule row by row: chord(last, first) <= 1.5 * max(chord(first, second), chord(last but one, last)) on the
    rows whose four end cells are finite; cyclic when more than half of them say yes."""
    lat, lon = np.asarray(lat2d, dtype=np.float64), np.asarray(lon2d, dtype=np.float64)
    nj, ni = lat.shape
    if ni < 3:
        return False
    yes = rows = 0
    for j in range(nj):
        ends = [0, 1, ni - 2, ni - 1]
        if not (np.all(np.isfinite(lat[j, ends])) and np.all(np.isfinite(lon[j, ends]))):
            continue
        p = [_xyz(lat[j, e], lon[j, e]) for e in ends]
        chord = lambda a, b: float(np.sqrt(np.sum((a - b) ** 2)))
        rows += 1
        yes += chord(p[3], p[0]) <= 1.5 * max(chord(p[0], p[1]), chord(p[2], p[3]))
    return rows > 0 and 2 * yes > rows


def box_ref(lat2d, lon2d, box, cyclic='auto'):
    """`curvilinear_box` by the statement -> (j0, nj_sel, i0, ni_sel, n_inside)."""
    row_any, col_any, n = flags_ref(lat2d, lon2d, box)
    if n == 0:
        raise ValueError('no cell lies within the box')
    cyc = cyclic_ref(lat2d, lon2d) if cyclic == 'auto' else bool(cyclic)
    return windows_ref(row_any, col_any, cyc) + (n,)


def index_ref(a, j0, nj_sel, i0, ni_sel, jax=-2, iax=-1):
    """The cut of an array along its row axis `jax` and / or column axis `iax` (None: the array has no such axis)."""
    a = np.asarray(a)
    if jax is not None:
        a = np.take(a, np.arange(j0, j0 + nj_sel), axis=jax)
    if iax is not None:
        a = np.take(a, (i0 + np.arange(ni_sel)) % a.shape[iax], axis=iax)
    return a


# ------------------------------------------------------------------------------- grids
def ocean_grid(nj, ni, dtype=np.float64):
    """The sheared global ocean grid of `synthetic.make_ocean_grid_case` (longitudes 0 ... 360) -> (lat2d, lon2d)."""
    from pgw4era5_amd import synthetic
    oc = synthetic.make_ocean_grid_case(nj=nj, ni=ni, ntime=1, land_patches=0)
    return oc['latitude'].astype(dtype), oc['longitude'].astype(dtype)


def grid_kinds(nj, ni):
    """name -> (lat2d, lon2d, cyclic): the global grid, the grid with two columns removed at each end (a gap: not cyclic)
    and the grid with two duplicated halo columns appended (NEMO / MPI-ESM style: cyclic)."""
    lat, lon = ocean_grid(nj, ni)
    return {'global': (lat, lon, True),
            'trimmed': (lat[:, 2:-2].copy(), lon[:, 2:-2].copy(), False),
            'halo': (np.concatenate([lat, lat[:, :2]], axis=1), np.concatenate([lon, lon[:, :2]], axis=1), True)}


def regional_grid(nj=14, ni=22, dtype=np.float64):
    """A rotated-pole-like regional grid over Europe: rows and columns slightly sheared, lon 2 ... 45, lat 30 ... 62."""
    j, i = np.meshgrid(np.arange(nj) / (nj - 1.0), np.arange(ni) / (ni - 1.0), indexing='ij')
    lat = 30.0 + 30.0 * j + 2.0 * np.sin(np.pi * i)
    lon = 5.0 + 38.0 * i + 3.0 * (j - 0.5) * (i - 0.5) * 2.0
    return lat.astype(dtype), lon.astype(dtype)


def scatter_grid(nj, ni, dtype, seed):
    """Coordinates without any structure - the marker does not need one: lat in [-90, 90], lon in [-400, 800], a tenth of the
    cells NaN or +-inf in lat, in lon or in both."""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-90.0, 90.0, (nj, ni)).astype(dtype)
    lon = rng.uniform(-400.0, 800.0, (nj, ni)).astype(dtype)
    bad = np.array([np.nan, np.inf, -np.inf], dtype=dtype)
    for a in (lat, lon):
        m = rng.random((nj, ni)) < 0.07
        a[m] = rng.choice(bad, size=int(m.sum()))
    return lat, lon


def sprinkle(lat, lon, seed):
    """Copies of the grid with NaN and +-inf coordinates sprinkled in."""
    rng = np.random.default_rng(seed)
    lat, lon = lat.copy(), lon.copy()
    bad = np.array([np.nan, np.inf, -np.inf], dtype=lat.dtype)
    for a in (lat, lon):
        m = rng.random(a.shape) < 0.07
        a[m] = rng.choice(bad, size=int(m.sum()))
    return lat, lon


def edge_grid(dtype, box=REF_BOX):
    """(lat2d, lon2d, table) of shape (6, 9): cells exactly on the four edges of `box` - the longitude edges reached with
    k = -1, 0 and +1 (287 and 397, -73 and 37, -433 and -323 for the box -73 ... 37) - and for each of them the neighbour
    one ulp of `dtype` outside and the one inside; the rest of the grid lies far outside.  table: a list of
    (flat index, edge name, 'on' | 'out' | 'in')."""
    lon1, lon2, lat1, lat2 = box
    lat_lo, lat_hi = min(lat1, lat2), max(lat1, lat2)
    mid_lat, mid_lon = dtype(0.5 * (lat_lo + lat_hi)), dtype(0.5 * (lon1 + lon2))
    t = dtype
    pts, table = [], []

    def add(lat, lon, edge, kind):
        table.append((len(pts), edge, kind))
        pts.append((t(lat), t(lon)))

    for edge, v, outward in (('lat_lo', lat_lo, -np.inf), ('lat_hi', lat_hi, np.inf)):
        v = t(v)
        assert float(v) == (lat_lo if edge == 'lat_lo' else lat_hi)                # the edge is a number of this dtype
        add(v, mid_lon, edge, 'on')
        add(np.nextafter(v, t(outward)), mid_lon, edge, 'out')
        add(np.nextafter(v, t(-outward)), mid_lon, edge, 'in')
    for k in (-1, 0, 1):                                           # lon + 360 k lies on the edge
        for edge, v, outward in (('lon1', lon1, -np.inf), ('lon2', lon2, np.inf)):
            v = t(v - 360.0 * k)
            assert float(v) + 360.0 * k == (lon1 if edge == 'lon1' else lon2)
            add(mid_lat, v, edge, 'on')
            add(mid_lat, np.nextafter(v, t(outward)), edge, 'out')
            add(mid_lat, np.nextafter(v, t(-outward)), edge, 'in')
    nj, ni = 6, 9
    assert len(pts) <= nj * ni
    lat = np.full(nj * ni, t(lat_hi + 40.0), dtype=dtype)          # far outside in latitude
    lon = np.full(nj * ni, mid_lon, dtype=dtype)
    for n, (a, b) in enumerate(pts):
        lat[n], lon[n] = a, b
    return lat.reshape(nj, ni), lon.reshape(nj, ni), table


def edge_expectation(table):
    """flat index -> inside?: on the edge and one ulp inside are inside, one ulp outside is not.  (A longitude one ulp
    outside lon1 is tried with the next k and then lies beyond lon2, the box being narrower than 360 degrees.)"""
    return {n: kind != 'out' for n, _, kind in table}


# ------------------------------------------------------------------------------- files
UNITS = 'days since 1850-01-01 00:00:00'
MONTHS = np.array([15.5, 45.0, 74.5, 105.0, 135.5, 166.0, 196.5, 227.5, 258.0, 288.5, 319.0, 349.5]) + 365.0 * 150   # noleap 2000
FILL = 1.0e20


def write_ocean_file(path, var='tos', nj=40, ni=60, times=MONTHS, dtype=np.float32, seed=0, scale=1.0):
    """An Omon-like NetCDF-3 file: `var` (time, j, i) of `dtype` with `_FillValue` 1e20 over land, 2-D latitude / longitude
    (float64), vertices_latitude / vertices_longitude (j, i, vertices), the index coordinates j and i, a cell-area field
    (j, i), time_bnds and one unrelated variable.  Returns dict(lat, lon, values as written)."""
    from pgw4era5_amd import ncio, synthetic
    F = ncio.Field
    times = np.asarray(times, dtype=np.float64)
    oc = synthetic.make_ocean_grid_case(nj=nj, ni=ni, ntime=len(times), seed=seed)
    lat, lon = oc['latitude'], oc['longitude']
    rng = np.random.default_rng(seed + 100)
    vals = scale * (oc['values'] + 0.01 * rng.standard_normal(oc['values'].shape))
    vals = np.where(np.isnan(vals), FILL, vals).astype(dtype)
    corner = np.array([[-1.0, -1.0], [-1.0, 1.0], [1.0, 1.0], [1.0, -1.0]])
    ds = ncio.Dataset(attrs={'source_id': 'TEST-OGCM', 'Conventions': 'CF-1.7', 'grid_label': 'gn'}, record_dim='time')
    ds['time'] = F(times, ('time',), {}, {'units': UNITS, 'calendar': 'noleap', 'standard_name': 'time', 'bounds': 'time_bnds'})
    ds['time_bnds'] = F(np.stack([times - 15.0, times + 15.0], axis=1), ('time', 'bnds'), {}, {})
    ds['j'] = F(np.arange(nj, dtype=np.int32), ('j',), {}, {'units': '1', 'long_name': 'cell index along second dimension'})
    ds['i'] = F(np.arange(ni, dtype=np.int32), ('i',), {}, {'units': '1', 'long_name': 'cell index along first dimension'})
    ds['latitude'] = F(lat, ('j', 'i'), {}, {'units': 'degrees_north', 'bounds': 'vertices_latitude'})
    ds['longitude'] = F(lon, ('j', 'i'), {}, {'units': 'degrees_east', 'bounds': 'vertices_longitude'})
    ds['vertices_latitude'] = F(lat[:, :, None] + 0.4 * corner[None, None, :, 0], ('j', 'i', 'vertices'), {}, {'units': 'degrees_north'})
    ds['vertices_longitude'] = F(lon[:, :, None] + 0.4 * corner[None, None, :, 1], ('j', 'i', 'vertices'), {}, {'units': 'degrees_east'})
    ds['areacello'] = F((1.0e9 * np.cos(np.deg2rad(lat))).astype(np.float32), ('j', 'i'), {}, {'units': 'm2'})
    ds['crs'] = F(np.array([4326], dtype=np.int32), ('one',), {}, {'grid_mapping_name': 'latitude_longitude'})
    ds[var] = F(vals, ('time', 'j', 'i'), {}, {'units': 'degC', '_FillValue': dtype(FILL), 'missing_value': dtype(FILL),
                                               'coordinates': 'latitude longitude', 'long_name': 'Sea Surface Temperature'})
    ncio.to_netcdf(ds, path)
    return dict(lat=lat, lon=lon, values=vals, land=oc['land'])


def write_regional_file(path, var='ta', nt=3, plev=(100000.0, 85000.0, 50000.0), seed=0):
    """A regional-model file: `var` (time, plev, rlat, rlon) float32, 2-D lat / lon (rlat, rlon) float32, the rotated
    coordinates rlat / rlon and a scalar grid-mapping variable."""
    from pgw4era5_amd import ncio
    F = ncio.Field
    lat, lon = regional_grid(dtype=np.float32)
    nj, ni = lat.shape
    rng = np.random.default_rng(seed)
    vals = (250.0 + 30.0 * rng.standard_normal((nt, len(plev), nj, ni))).astype(np.float32)
    vals[rng.random(vals.shape) < 0.1] = np.float32(FILL)
    times = MONTHS[:nt]
    ds = ncio.Dataset(attrs={'source_id': 'TEST-RCM'}, record_dim='time')
    ds['time'] = F(times, ('time',), {}, {'units': UNITS, 'calendar': 'noleap'})
    ds['plev'] = F(np.asarray(plev, dtype=np.float64), ('plev',), {}, {'units': 'Pa'})
    ds['rlat'] = F(np.linspace(-7.0, 7.0, nj), ('rlat',), {}, {'units': 'degrees', 'standard_name': 'grid_latitude'})
    ds['rlon'] = F(np.linspace(-11.0, 11.0, ni), ('rlon',), {}, {'units': 'degrees', 'standard_name': 'grid_longitude'})
    ds['lat'] = F(lat, ('rlat', 'rlon'), {}, {'units': 'degrees_north'})
    ds['lon'] = F(lon, ('rlat', 'rlon'), {}, {'units': 'degrees_east'})
    ds['rotated_pole'] = F(np.array([0], dtype=np.int32), ('one',), {}, {'grid_mapping_name': 'rotated_latitude_longitude'})
    ds[var] = F(vals, ('time', 'plev', 'rlat', 'rlon'), {}, {'units': 'K', '_FillValue': np.float32(FILL), 'grid_mapping': 'rotated_pole'})
    ncio.to_netcdf(ds, path)
    return dict(lat=lat, lon=lon, values=vals)


def read_raw(path):
    """name -> (big-endian data as the file holds it, dimensions, attributes), the global attributes, the record dimensions."""
    from scipy.io import netcdf_file
    out = {}
    with netcdf_file(path, 'r', mmap=False) as nc:
        for name, v in nc.variables.items():
            out[name] = (np.array(v.data, copy=True), tuple(v.dimensions), dict(v._attributes))
        gatts = dict(nc._attributes)
        rec = [d for d, n in nc.dimensions.items() if n is None]
    return out, gatts, rec


def same_attrs(a, b):
    if list(a) != list(b):
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def words(a):
    """The array's words as unsigned integers of its own byte order (indexing them moves integers, not values)."""
    a = np.ascontiguousarray(a)
    return a.view(np.dtype('u%d' % a.dtype.itemsize).newbyteorder(a.dtype.byteorder))
