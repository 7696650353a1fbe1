"""GPU checks of step_01's level selection, lon-lat box and model-top merge: the kernel behind `pgw_select_box` and the
layer above it in pgw4era5_amd/step_01_extract_deltas.py (select, select_file, merge_levels_files,
climatology_files(box=...), the sub-commands `select` and `merge_levels`).

`cdo` is not available (extract_climate_delta.sh:194-208, CFday_cut_subdomain.sh:28-30 and
Emon_add_top_from_Amon.sh:45-56 call it), so the definition of correct is the numpy index statement `index_ref` below plus
the documented rules of `lonlat_box` / `level_indices`.  The kernel moves words, so EVERY comparison is bit equality on
unsigned-integer views (or on the bytes of a file): no tolerance anywhere."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
PGW_ERR_ARG = 2


def index_ref(src, lev_index, lat0, nlat_sel, lon0, nlon_sel):
    """The definition: dst[r, k, i, j] = src[r, lev_index[k], lat0 + i, (lon0 + j) % nlon_src]."""
    cols = (lon0 + np.arange(nlon_sel)) % src.shape[3]
    lev = np.arange(src.shape[1]) if lev_index is None else np.asarray(lev_index)
    return src[:, lev][:, :, lat0:lat0 + nlat_sel][:, :, :, cols]


def bit_patterns(shape, elem_bytes, seed):
    """Random words with the patterns a value-based copy would damage sprinkled in: all ones, signalling and quiet NaNs
    with payloads, infinities, -0, the short / float fill values."""
    rng = np.random.default_rng(seed)
    u = UINT[elem_bytes]
    x = rng.integers(0, 2**(8 * elem_bytes), size=shape, dtype=u, endpoint=False)
    special = {2: [0xFFFF, 0x8000, 0x7FFF, 0x0000, 0x8001],
               4: [0xFFFFFFFF, 0x7FC00001, 0x7F800001, 0xFFC12345, 0x7F800000, 0x80000000, 0x7E967699],
               8: [0xFFFFFFFFFFFFFFFF, 0x7FF8000000000001, 0x7FF0000000000001, 0xFFF8123456789ABC, 0x7FF0000000000000,
                   0x8000000000000000, 0x479E17B84357691B]}[elem_bytes]
    flat = x.reshape(-1)
    where = rng.random(flat.shape) < 0.2
    flat[where] = rng.choice(np.array(special, dtype=u), size=int(where.sum()))
    return x


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    return default_context()


@pytest.fixture(scope='module')
def s1():
    from pgw4era5_amd import step_01_extract_deltas
    return step_01_extract_deltas


def to_dev(ctx, s1, host):
    d = ctx.empty(host.shape, host.dtype)
    s1._upload_words(ctx, d, host)
    return d


def run(ctx, s1, d_src, lev_index, lat0, nlat_sel, lon0, nlon_sel, d_dst=None, lev_dst0=0):
    """One pgw_select_box launch on the device source (nrec, nlev, nlat, nlon) -> the destination on the host."""
    nrec, nlev, nlat, nlon = d_src.shape
    nsel = nlev if lev_index is None else len(lev_index)
    if d_dst is None:
        d_dst = ctx.empty((nrec, nsel, nlat_sel, nlon_sel), d_src.dtype)
    s1._launch_select(ctx, d_src.dtype.itemsize, nrec, nlev, nlat, nlon, d_src.ptr, lev_index, (lat0, nlat_sel), (lon0, nlon_sel),
                      d_dst.shape[1], lev_dst0, d_dst.ptr)
    return d_dst.numpy()


def lon_windows(n):
    """(lon0, nlon_sel): no wrap, wrap, the full circle from a column other than 0, single columns, rows of 1 / 63 / 64 / 65
    columns with and without wrap, multiples of 8 from a multiple of 8 (the widest per-lane form of every element size), and
    at n = 257 rows longer than a block of 256 threads."""
    w = {(0, n), (0, 1), (n - 1, 1), (n // 3, n), (n // 2, max(n // 2, 1))}
    for s in (1, 63, 64, 65):
        if s <= n:
            w.add((min(2, n - s), s))                 # no wrap
            w.add((n - 1, s))                         # wraps after one column (s > 1)
    if n >= 64:
        w.add((8, 48)); w.add((n - n % 8 - 8, 48)); w.add((n - 3, 7))
    return sorted(w)


LAT_WINDOWS = {1: [(0, 1)], 7: [(0, 1), (6, 1), (2, 3), (0, 7)]}
LEVEL_LISTS = {1: [None, [0]], 5: [None, [0, 2, 4], [3, 0, 4, 1], [2]]}      # all, every second, reversed and shuffled, one


# ------------------------------------------------------------------------------- 1. the kernel against the index statement
@pytest.mark.parametrize('nlon_src', [1, 5, 64, 65, 130, 257])
@pytest.mark.parametrize('nrec', [1, 3])
@pytest.mark.parametrize('elem_bytes', [2, 4, 8])
def test_kernel_vs_numpy(ctx, s1, elem_bytes, nrec, nlon_src):
    n_checked = 0
    for nlev, nlat in ((5, 7), (1, 7), (5, 1)):
        src = bit_patterns((nrec, nlev, nlat, nlon_src), elem_bytes, seed=1000 * elem_bytes + 100 * nrec + nlon_src + nlev + nlat)
        d_src = to_dev(ctx, s1, src)
        for lon0, nlon_sel in lon_windows(nlon_src):
            for lat0, nlat_sel in LAT_WINDOWS[nlat]:
                for lev in LEVEL_LISTS[nlev]:
                    got = run(ctx, s1, d_src, lev, lat0, nlat_sel, lon0, nlon_sel)
                    want = index_ref(src, lev, lat0, nlat_sel, lon0, nlon_sel)
                    assert got.dtype == src.dtype and got.shape == want.shape
                    assert np.array_equal(got, want), (nlev, nlat, lon0, nlon_sel, lat0, nlat_sel, lev)
                    n_checked += 1
    assert n_checked >= 28


def test_many_rows_and_a_float_view(ctx, s1):
    """More output rows than one pass of the grid holds (blocks stride over the row tiles), and the array-level `select`
    on a float32 array with NaN payloads: the same dtype comes back, bits untouched."""
    # 2 * 2 * 5000 rows of 257 two-byte words from an odd column: one row per block and pass of four, 5000 row tiles on
    # a grid of at most 4096 blocks
    src = bit_patterns((2, 2, 5100, 259), 2, seed=7)
    got = run(ctx, s1, to_dev(ctx, s1, src), None, 50, 5000, 5, 257)
    assert np.array_equal(got, index_ref(src, None, 50, 5000, 5, 257))
    f = bit_patterns((2, 4, 6, 12), 4, seed=8).view(np.float32)
    plev = np.array([100000.0, 85000.0, 50000.0, 25000.0])
    lat, lon = np.array([75.0, 45.0, 15.0, -15.0, -45.0, -75.0]), np.arange(0.0, 360.0, 30.0)
    out = s1.select(f, levels=[25000, 100000], box=(-73, 37, -42, 34), plev=plev, lat=lat, lon=lon)
    assert out.dtype == np.float32
    assert np.array_equal(out.view(np.uint32), index_ref(f.view(np.uint32), [0, 3], 2, 2, 10, 4))
    big = f.astype('>f4')                                            # any byte order: words are words
    out = s1.select(big, box=(-73, 37, -42, 34), lat=lat, lon=lon)   # no plev: (..., lat, lon) with the levels folded
    assert out.dtype == big.dtype and out.tobytes() == np.ascontiguousarray(big[:, :, 2:4][..., [10, 11, 0, 1]]).tobytes()
    d = s1.select(to_dev(ctx, s1, f), levels=[50000], plev=plev)
    assert d.shape == (2, 1, 6, 12) and np.array_equal(d.numpy().view(np.uint32), f.view(np.uint32)[:, 2:3])


# ------------------------------------------------------------------------------- 2. only the addressed slab; the merge
@pytest.mark.parametrize('elem_bytes', [2, 4, 8])
@pytest.mark.parametrize('lev_dst0', [0, 2])
def test_only_the_addressed_slab_is_written(ctx, s1, elem_bytes, lev_dst0):
    u = UINT[elem_bytes]
    sentinel = u(0xA5A5A5A5A5A5A5A5 & (2**(8 * elem_bytes) - 1))
    src = bit_patterns((3, 5, 7, 65), elem_bytes, seed=31 + elem_bytes)
    src[src == sentinel] = 0
    lev, (lat0, nlat_sel, lon0, nlon_sel) = [4, 0, 2], (2, 3, 60, 9)
    dst = np.full((3, 6, nlat_sel, nlon_sel), sentinel, dtype=u)
    got = run(ctx, s1, to_dev(ctx, s1, src), lev, lat0, nlat_sel, lon0, nlon_sel, d_dst=to_dev(ctx, s1, dst), lev_dst0=lev_dst0)
    assert np.array_equal(got[:, lev_dst0:lev_dst0 + 3], index_ref(src, lev, lat0, nlat_sel, lon0, nlon_sel))
    rest = np.delete(got, np.arange(lev_dst0, lev_dst0 + 3), axis=1)
    assert rest.shape[1] == 3 and np.all(rest == sentinel)
    # two launches into one destination are the merge
    a, b = src, bit_patterns((3, 3, 7, 65), elem_bytes, seed=77 + elem_bytes)
    d_dst = to_dev(ctx, s1, np.full((3, 6, nlat_sel, nlon_sel), sentinel, dtype=u))
    run(ctx, s1, to_dev(ctx, s1, a), [0, 1, 3], lat0, nlat_sel, lon0, nlon_sel, d_dst=d_dst, lev_dst0=0)
    merged = run(ctx, s1, to_dev(ctx, s1, b), None, lat0, nlat_sel, lon0, nlon_sel, d_dst=d_dst, lev_dst0=3)
    want = np.concatenate([index_ref(a, [0, 1, 3], lat0, nlat_sel, lon0, nlon_sel), index_ref(b, None, lat0, nlat_sel, lon0, nlon_sel)], axis=1)
    assert np.array_equal(merged, want)


# ------------------------------------------------------------------------------- 3. every form gives the same bytes
@pytest.mark.parametrize('elem_bytes', [2, 4, 8])
def test_forms_give_the_same_bytes(ctx, s1, elem_bytes):
    # (nlon_src, lon0, nlon_sel): 16 bytes per lane possible for every element size (multiples of 8, with and without wrap);
    # possible for the short elements only (multiples of 2 / 4); not possible at all (odd)
    shapes = [(64, 8, 48), (64, 40, 48), (128, 0, 128), (130, 2, 64), (132, 4, 8), (65, 3, 17), (64, 7, 48), (64, 8, 47)]
    for nlon_src, lon0, nlon_sel in shapes:
        src = bit_patterns((3, 5, 7, nlon_src), elem_bytes, seed=nlon_src + lon0 + elem_bytes)
        d_src = to_dev(ctx, s1, src)
        want = index_ref(src, [3, 0, 4, 1], 1, 5, lon0, nlon_sel)
        default = run(ctx, s1, d_src, [3, 0, 4, 1], 1, 5, lon0, nlon_sel)
        assert np.array_equal(default, want)
        for knob in ('force_vec1', 'force_off64'):
            old = ctx.set_option(knob, 1)
            try:
                forced = run(ctx, s1, d_src, [3, 0, 4, 1], 1, 5, lon0, nlon_sel)
            finally:
                ctx.set_option(knob, old)
            assert forced.tobytes() == default.tobytes(), (knob, nlon_src, lon0, nlon_sel)
    # a destination that starts 4 bytes into its allocation: the pointers decide the form too
    if elem_bytes == 4:
        src = bit_patterns((2, 2, 3, 64), 4, seed=5)
        d_src = to_dev(ctx, s1, src)
        buf = ctx.empty((2 * 2 * 3 * 64 + 1,), np.uint32)
        from pgw4era5_amd.device import DeviceArray
        off = DeviceArray(ctx, (2, 2, 3, 64), np.uint32, ptr=buf.ptr + 4, owner=buf)
        assert np.array_equal(run(ctx, s1, d_src, None, 0, 3, 8, 64, d_dst=off), index_ref(src, None, 0, 3, 8, 64))


# ------------------------------------------------------------------------------- 4. argument errors
def test_argument_errors(ctx, s1):
    import ctypes as C
    lib = ctx.lib
    sentinel = np.uint32(0xA5A5A5A5)
    src = bit_patterns((2, 5, 7, 16), 4, seed=3)
    d_src = to_dev(ctx, s1, src)
    d_dst = to_dev(ctx, s1, np.full((2, 6, 7, 16), sentinel, dtype=np.uint32))

    def call(elem_bytes=4, nrec=2, nlev_src=5, nlat_src=7, nlon_src=16, src_ptr=d_src.ptr, lev=(0, 1, 2), lat0=0, nlat_sel=7, lon0=0,
             nlon_sel=16, nlev_dst=6, lev_dst0=0, dst_ptr=d_dst.ptr, nlev_sel=None):
        arr = None if lev is None else np.ascontiguousarray(lev, dtype=np.int32)
        p = None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int))
        nsel = nlev_sel if nlev_sel is not None else len(arr)
        rc = lib.pgw_select_box(ctx.handle, elem_bytes, nrec, nlev_src, nlat_src, nlon_src, src_ptr, nsel, p, lat0, nlat_sel, lon0,
                                nlon_sel, nlev_dst, lev_dst0, dst_ptr)
        return rc, (lib.pgw_last_error(ctx.handle) or b'').decode()

    bad = [(dict(elem_bytes=3), 'elem_bytes must be 2, 4 or 8'), (dict(elem_bytes=1), 'elem_bytes must be 2, 4 or 8'),
           (dict(elem_bytes=16), 'elem_bytes must be 2, 4 or 8'),
           (dict(nrec=0), 'must be positive'), (dict(nlon_src=0, lon0=0, nlon_sel=1), 'must be positive'),
           (dict(lev=(0, 5)), 'lev_index must lie in [0, nlev_src)'), (dict(lev=(-1,)), 'lev_index must lie in [0, nlev_src)'),
           (dict(lat0=-1), 'lat0'), (dict(lat0=1), 'lat0'), (dict(lat0=3, nlat_sel=5), 'lat0'), (dict(nlat_sel=0), 'lat0'),
           (dict(lon0=-1), 'lon0 must lie in [0, nlon_src)'), (dict(lon0=16), 'lon0 must lie in [0, nlon_src)'),
           (dict(nlon_sel=0), 'nlon_sel must be in [1, nlon_src]'), (dict(nlon_sel=17), 'nlon_sel must be in [1, nlon_src]'),
           (dict(lev_dst0=4), 'lev_dst0 + nlev_sel must not exceed nlev_dst'), (dict(lev_dst0=-1), 'lev_dst0 + nlev_sel must not exceed nlev_dst'),
           (dict(nlev_dst=2), 'lev_dst0 + nlev_sel must not exceed nlev_dst'),
           (dict(lev=tuple([0] * 257), nlev_dst=300), 'nlev_sel must be in [1, 256]'), (dict(lev=None, nlev_sel=0), 'nlev_sel must be in [1, 256]'),
           (dict(lev=None, nlev_sel=6), 'without lev_index nlev_sel must not exceed nlev_src'),
           (dict(src_ptr=None), 'null pointer'), (dict(dst_ptr=None), 'null pointer'),
           (dict(src_ptr=d_src.ptr + 2), 'aligned'), (dict(dst_ptr=d_src.ptr, nlev_dst=5, lev=(0,)), 'must not overlap')]
    for kw, text in bad:
        rc, msg = call(**kw)
        assert rc == PGW_ERR_ARG, (kw, rc, msg)
        assert msg.startswith('pgw_select_box: ') and text in msg, (kw, msg)
    # nothing was launched: source and destination are as they were
    assert np.all(d_dst.numpy() == sentinel) and np.array_equal(d_src.numpy(), src)
    # the Python layer turns the status into a ValueError with that message
    with pytest.raises(ValueError, match='nlon_sel must be in'):
        s1._launch_select(ctx, 4, 2, 5, 7, 16, d_src.ptr, None, (0, 7), (0, 17), 6, 0, d_dst.ptr)
    rc, msg = call()
    assert rc == 0
    got = d_dst.numpy()
    assert np.array_equal(got[:, :3], src[:, :3]) and np.all(got[:, 3:] == sentinel)


# ------------------------------------------------------------------------------- files
UNITS = 'days since 1850-01-01 00:00:00'
PLEV = np.array([100000.0, 85000.0, 50000.0, 25000.0])
LAT = np.array([75.0, 45.0, 15.0, -15.0, -45.0, -75.0])
LON = np.arange(0.0, 360.0, 30.0)
BOX = (-73.0, 37.0, -42.0, 34.0)              # wraps across 0 deg: columns 300, 330, 0, 30 -> 10, 11, 0, 1; rows 15, -15 -> 2, 3
BOX_ROWS, BOX_COLS, BOX_LON = slice(2, 4), np.array([10, 11, 0, 1]), np.array([-60.0, -30.0, 0.0, 30.0])


def bnds(c):
    c = np.asarray(c, dtype=np.float64)
    half = 0.5 * np.abs(c[1] - c[0]) if len(c) > 1 else 1.0
    return np.stack([c - half, c + half], axis=1)


def write_file(path, var, values, times, vattrs, plev=PLEV, lat=LAT, lon=LON, extra=None, calendar='noleap'):
    """A NetCDF-3 file with `var` on (time, [plev,] lat, lon), the coordinates, their bounds and one unrelated variable."""
    from pgw4era5_amd import ncio
    ds = ncio.Dataset(attrs={'source_id': 'TEST-GCM', 'Conventions': 'CF-1.7'}, record_dim='time')
    times = np.asarray(times, dtype=np.float64)
    ds['time'] = ncio.Field(times, ('time',), {}, {'units': UNITS, 'calendar': calendar, 'standard_name': 'time'})
    if values.ndim == 4:
        ds['plev'] = ncio.Field(plev, ('plev',), {}, {'units': 'Pa', 'positive': 'down', 'bounds': 'plev_bnds'})
        ds['plev_bnds'] = ncio.Field(bnds(plev), ('plev', 'bnds'), {}, {})
    ds['lat'] = ncio.Field(lat, ('lat',), {}, {'units': 'degrees_north', 'bounds': 'lat_bnds'})
    ds['lon'] = ncio.Field(lon, ('lon',), {}, {'units': 'degrees_east', 'bounds': 'lon_bnds'})
    ds['lat_bnds'] = ncio.Field(bnds(lat), ('lat', 'bnds'), {}, {})
    ds['lon_bnds'] = ncio.Field(bnds(lon), ('lon', 'bnds'), {}, {})
    ds['crs'] = ncio.Field(np.array([4326], dtype=np.int32), ('one',), {}, {'grid_mapping_name': 'latitude_longitude'})
    for name, f in (extra or {}).items():
        ds[name] = f
    dims = ('time', 'plev', 'lat', 'lon') if values.ndim == 4 else ('time', 'lat', 'lon')
    ds[var] = ncio.Field(values, dims, {}, vattrs)
    ncio.to_netcdf(ds, path)
    return path


def read_raw(path):
    """name -> (big-endian data as the file holds it, dimensions, attributes) through scipy's reader."""
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
    """The array's words as unsigned integers OF ITS OWN BYTE ORDER: equal values are equal bytes in the file, and indexing
    or concatenating the result moves integers (numpy would convert floats of the file's byte order by value)."""
    a = np.ascontiguousarray(a)
    return a.view(np.dtype('u%d' % a.dtype.itemsize).newbyteorder(a.dtype.byteorder))


def case_values(kind, seed=11, nt=3):
    """(values (nt, 4, 6, 12), attributes) of the three NetCDF types covered."""
    rng = np.random.default_rng(seed)
    shape = (nt, 4, 6, 12)
    if kind == 'f4_fill':
        v = (rng.standard_normal(shape) * 30 + 250).astype(np.float32)
        v[rng.random(shape) < 0.15] = np.float32(1.0e20)
        return v, {'units': 'K', '_FillValue': np.float32(1.0e20), 'missing_value': np.float32(1.0e20), 'long_name': 'Air Temperature'}
    if kind == 'f8':
        return rng.standard_normal(shape) * 30 + 250, {'units': 'K', 'cell_methods': 'time: mean'}
    v = rng.integers(-32767, 32768, size=shape).astype(np.int16)
    v[rng.random(shape) < 0.1] = np.int16(-32768)
    return v, {'units': 'K', 'scale_factor': np.float64(0.01), 'add_offset': np.float64(250.0), '_FillValue': np.int16(-32768)}


# ------------------------------------------------------------------------------- 5. select_file
@pytest.mark.parametrize('kind', ['f4_fill', 'f8', 'i2_packed'])
def test_select_file_bytes(s1, tmp_path, kind):
    values, vattrs = case_values(kind)
    tas = ncio_field_tas()
    inp = write_file(str(tmp_path / 'in.nc'), 'ta', values, [15.5, 45.0, 74.5], vattrs, extra={'tas': tas})
    out = s1.select_file(inp, str(tmp_path / 'out.nc'), 'ta', levels=[25000, 100000], box=BOX)
    assert out == str(tmp_path / 'out.nc')
    a, ga, reca = read_raw(inp)
    b, gb, recb = read_raw(out)
    assert list(a) == list(b) and same_attrs(ga, gb) and reca == recb == ['time']
    lev = [0, 3]
    # the variable: raw data = the index expression of the input's raw data; type, dimensions and attributes unchanged
    assert b['ta'][0].dtype == a['ta'][0].dtype and b['ta'][1] == a['ta'][1] and same_attrs(a['ta'][2], b['ta'][2])
    assert np.array_equal(words(b['ta'][0]), words(a['ta'][0])[:, lev][:, :, BOX_ROWS][..., BOX_COLS])
    # coordinates and bounds cut / shifted
    assert np.array_equal(b['plev'][0], PLEV[lev]) and np.array_equal(b['plev_bnds'][0], a['plev_bnds'][0][lev])
    assert np.array_equal(b['lat'][0], LAT[BOX_ROWS]) and np.array_equal(b['lat_bnds'][0], a['lat_bnds'][0][BOX_ROWS])
    assert np.array_equal(b['lon'][0], BOX_LON)
    assert np.array_equal(b['lon_bnds'][0], a['lon_bnds'][0][BOX_COLS] + np.array([-360.0, -360.0, 0.0, 0.0])[:, None])
    # another variable on lat / lon is cut with the same indices; everything else is carried over
    assert np.array_equal(words(b['tas'][0]), words(a['tas'][0])[:, BOX_ROWS][..., BOX_COLS]) and same_attrs(a['tas'][2], b['tas'][2])
    for name in ('time', 'crs'):
        assert np.array_equal(words(a[name][0]), words(b[name][0])) and same_attrs(a[name][2], b[name][2])
    for name in a:
        assert same_attrs(a[name][2], b[name][2]) and a[name][1] == b[name][1]
    # identity box and all levels: the variable's bytes are the input's
    ident = s1.select_file(inp, str(tmp_path / 'ident.nc'), 'ta', levels=PLEV[::-1].tolist(), box=(0, 360, -90, 90))
    c, _, _ = read_raw(ident)
    assert c['ta'][0].tobytes() == a['ta'][0].tobytes()
    for name in a:
        assert c[name][0].tobytes() == a[name][0].tobytes(), name
    # the output does not depend on max_records
    one = s1.select_file(inp, str(tmp_path / 'one.nc'), 'ta', levels=[25000, 100000], box=BOX, max_records=1)
    assert open(one, 'rb').read() == open(out, 'rb').read()
    # a variable without a level axis; only a box, only levels
    s1.select_file(inp, str(tmp_path / 'tas.nc'), 'tas', box=BOX)
    t, _, _ = read_raw(str(tmp_path / 'tas.nc'))
    assert np.array_equal(words(t['tas'][0]), words(a['tas'][0])[:, BOX_ROWS][..., BOX_COLS])
    assert np.array_equal(words(t['ta'][0]), words(a['ta'][0])[:, :, BOX_ROWS][..., BOX_COLS])       # cut on the host here
    s1.select_file(inp, str(tmp_path / 'lev.nc'), 'ta', levels=[50000])
    l, _, _ = read_raw(str(tmp_path / 'lev.nc'))
    assert np.array_equal(words(l['ta'][0]), words(a['ta'][0])[:, 2:3]) and np.array_equal(l['lon'][0], LON)
    with pytest.raises(ValueError, match='levels need'):
        s1.select_file(inp, str(tmp_path / 'x.nc'), 'tas', levels=[50000])
    with pytest.raises(ValueError, match='70000'):
        s1.select_file(inp, str(tmp_path / 'x.nc'), 'ta', levels=[70000])
    with pytest.raises(ValueError, match='must end in'):
        s1.select_file(inp, str(tmp_path / 'x.nc'), 'lon_bnds', box=BOX)


def ncio_field_tas():
    from pgw4era5_amd import ncio
    rng = np.random.default_rng(5)
    return ncio.Field((rng.standard_normal((3, 6, 12)) * 10 + 280).astype(np.float32), ('time', 'lat', 'lon'), {},
                      {'units': 'K', '_FillValue': np.float32(1.0e20)})


# ------------------------------------------------------------------------------- 6. merge_levels_files
EMON_PLEV = np.array([100000.0, 85000.0, 70000.0, 50000.0, 25000.0])
AMON_PLEV = np.array([7000.0, 5000.0, 1000.0])
MONTHS = np.array([15.5, 45.0, 74.5, 105.0, 135.5, 166.0, 196.5, 227.5, 258.0, 288.5, 319.0, 349.5]) + 365.0 * 150   # year 2000, noleap


@pytest.fixture()
def emon_amon(tmp_path):
    rng = np.random.default_rng(21)
    va = (rng.standard_normal((12, 5, 6, 12)) * 3).astype(np.float32)
    vb = (rng.standard_normal((12, 3, 6, 12)) * 3).astype(np.float32)
    va[rng.random(va.shape) < 0.1] = np.float32(1.0e20)
    attrs = {'units': 'K', '_FillValue': np.float32(1.0e20), 'long_name': 'Air Temperature'}
    d = str(tmp_path)
    a = write_file(os.path.join(d, 'emon.nc'), 'ta', va, MONTHS, attrs, plev=EMON_PLEV)
    b = write_file(os.path.join(d, 'amon.nc'), 'ta', vb, MONTHS, dict(attrs, long_name='from Amon'), plev=AMON_PLEV)
    return d, a, b, va, vb


def test_merge_levels_files(s1, emon_amon):
    from pgw4era5_amd import functions as F
    d, a, b, va, vb = emon_amon
    out = s1.merge_levels_files(a, b, os.path.join(d, 'ta_delta.nc'), 'ta', levels_a=[25000, 100000, 70000])
    ra, _, _ = read_raw(a)
    rb, _, _ = read_raw(b)
    ro, go, rec = read_raw(out)
    keep = [0, 2, 4]                                                  # file order, whatever the order of the request
    assert np.array_equal(words(ro['ta'][0]), np.concatenate([words(ra['ta'][0])[:, keep], words(rb['ta'][0])], axis=1))
    assert ro['ta'][0].dtype == ra['ta'][0].dtype and same_attrs(ro['ta'][2], ra['ta'][2]) and rec == ['time']
    assert np.array_equal(ro['plev'][0], np.concatenate([EMON_PLEV[keep], AMON_PLEV])) and same_attrs(ro['plev'][2], ra['plev'][2])
    assert np.array_equal(ro['plev_bnds'][0], np.concatenate([ra['plev_bnds'][0][keep], rb['plev_bnds'][0]]))
    for name in ('time', 'lat', 'lon', 'lat_bnds', 'lon_bnds', 'crs'):
        assert ro[name][0].tobytes() == ra[name][0].tobytes() and same_attrs(ro[name][2], ra[name][2])
    one = s1.merge_levels_files(a, b, os.path.join(d, 'one.nc'), 'ta', levels_a=[25000, 100000, 70000], max_records=1)
    assert open(one, 'rb').read() == open(out, 'rb').read()
    # levels_b, and both lists absent
    s1.merge_levels_files(a, b, os.path.join(d, 'm2.nc'), 'ta', levels_b=[1000, 7000])
    r2, _, _ = read_raw(os.path.join(d, 'm2.nc'))
    assert np.array_equal(words(r2['ta'][0]), np.concatenate([words(ra['ta'][0]), words(rb['ta'][0])[:, [0, 2]]], axis=1))
    # the result loads through load_delta: decoded (fill -> NaN), on the merged level axis
    every = F.load_delta(d, 'ta', np.datetime64('2000-03-10T00:00:00'))
    assert every.dims == ('time', 'plev', 'lat', 'lon') and every.shape == (12, 6, 6, 12)
    assert np.array_equal(np.asarray(every.coords['plev'], dtype=np.float64), np.concatenate([EMON_PLEV[keep], AMON_PLEV]))
    want = np.concatenate([va[:, keep], vb], axis=1)
    want = np.where(want == np.float32(1.0e20), np.float32(np.nan), want)
    got = np.asarray(every.values, dtype=np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    one_time = F.load_delta(d, 'ta', np.datetime64('2000-03-10T00:00:00'), np.datetime64('2000-03-10T00:00:00'))
    assert one_time.shape == (1, 6, 6, 12)


def test_merge_levels_files_errors(s1, emon_amon, tmp_path):
    d, a, b, va, vb = emon_amon
    attrs = {'units': 'K', '_FillValue': np.float32(1.0e20)}
    x = str(tmp_path / 'x.nc')
    overlap = write_file(str(tmp_path / 'ov.nc'), 'ta', vb, MONTHS, attrs, plev=np.array([25000.0, 5000.0, 1000.0]))
    with pytest.raises(ValueError, match='25000'):
        s1.merge_levels_files(a, overlap, x, 'ta')
    s1.merge_levels_files(a, overlap, x, 'ta', levels_b=[5000, 1000])          # the overlapping level is not selected: fine
    s1.merge_levels_files(a, overlap, x, 'ta', levels_a=[100000, 85000])
    moved = write_file(str(tmp_path / 't.nc'), 'ta', vb, MONTHS + 1.0, attrs, plev=AMON_PLEV)
    with pytest.raises(ValueError, match='time'):
        s1.merge_levels_files(a, moved, x, 'ta')
    fewer = write_file(str(tmp_path / 'f.nc'), 'ta', vb[:11], MONTHS[:11], attrs, plev=AMON_PLEV)
    with pytest.raises(ValueError, match='do not match'):
        s1.merge_levels_files(a, fewer, x, 'ta')
    other_lat = write_file(str(tmp_path / 'la.nc'), 'ta', vb, MONTHS, attrs, plev=AMON_PLEV, lat=LAT + 0.5)
    with pytest.raises(ValueError, match='lat'):
        s1.merge_levels_files(a, other_lat, x, 'ta')
    other_lon = write_file(str(tmp_path / 'lo.nc'), 'ta', vb, MONTHS, attrs, plev=AMON_PLEV, lon=LON + 1.0)
    with pytest.raises(ValueError, match='lon'):
        s1.merge_levels_files(a, other_lon, x, 'ta')
    f8 = write_file(str(tmp_path / 'd.nc'), 'ta', vb.astype(np.float64), MONTHS, {'units': 'K'}, plev=AMON_PLEV)
    with pytest.raises(ValueError, match='NetCDF types differ'):
        s1.merge_levels_files(a, f8, x, 'ta')
    with pytest.raises(ValueError, match='3000'):
        s1.merge_levels_files(a, b, x, 'ta', levels_b=[3000])


# ------------------------------------------------------------------------------- 7. climatology with a box
def test_climatology_with_box(s1, tmp_path):
    """Two input files (years 2000 and 2001, noleap, monthly), float32 with fill values -> NaN cells, a box that wraps."""
    rng = np.random.default_rng(9)
    attrs = {'units': 'K', '_FillValue': np.float32(1.0e20)}
    paths, cut_paths = [], []
    for y in range(2):
        v = (rng.standard_normal((12, 4, 6, 12)) * 30 + 250).astype(np.float32)
        v[rng.random(v.shape) < 0.2] = np.float32(1.0e20)
        v[:, 1, 2, 11] = np.float32(1.0e20)                          # a cell inside the box without any sample
        p = write_file(str(tmp_path / ('y%d.nc' % y)), 'ta', v, MONTHS + 365.0 * y, attrs)
        paths.append(p)
        cut_paths.append(s1.select_file(p, str(tmp_path / ('y%d_box.nc' % y)), 'ta', box=BOX))
    boxed = s1.climatology_files(paths, str(tmp_path / 'clim_box.nc'), 'ta', 'ymonmean', box=BOX)
    of_cut = s1.climatology_files(cut_paths, str(tmp_path / 'clim_of_cut.nc'), 'ta', 'ymonmean')
    whole = s1.climatology_files(paths, str(tmp_path / 'clim.nc'), 'ta', 'ymonmean')
    rb, gb, _ = read_raw(boxed)
    rc, gc, _ = read_raw(of_cut)
    rw, _, _ = read_raw(whole)
    # = the climatology of the cut files, bit for bit, variable by variable (and as whole files)
    assert list(rb) == list(rc) and same_attrs(gb, gc)
    for name in rb:
        assert rb[name][0].dtype == rc[name][0].dtype and rb[name][0].tobytes() == rc[name][0].tobytes(), name
        assert rb[name][1] == rc[name][1] and same_attrs(rb[name][2], rc[name][2]), name
    assert open(boxed, 'rb').read() == open(of_cut, 'rb').read()
    # = the un-boxed climatology cut with the same indices
    assert rb['ta'][0].shape == (12, 4, 2, 4)
    assert np.array_equal(words(rb['ta'][0]), words(rw['ta'][0])[:, :, BOX_ROWS][..., BOX_COLS])
    assert np.array_equal(rb['lon'][0], BOX_LON) and np.array_equal(rb['lat'][0], LAT[BOX_ROWS])
    assert np.array_equal(rb['lat_bnds'][0], rw['lat_bnds'][0][BOX_ROWS])
    assert np.all(rb['ta'][0][:, 1, 0, 1] == np.float32(1.0e20))       # source cell (lat 2, lon 11): no sample -> the fill value
    assert np.any(rb['ta'][0] != np.float32(1.0e20))
    # max_records does not matter, with or without the box
    again = s1.climatology_files(paths, str(tmp_path / 'clim_box1.nc'), 'ta', 'ymonmean', box=BOX, max_records=1)
    assert open(again, 'rb').read() == open(boxed, 'rb').read()
    # box=None is the call as it was: same file as without the keyword
    none = s1.climatology_files(paths, str(tmp_path / 'clim_none.nc'), 'ta', 'ymonmean', box=None)
    assert open(none, 'rb').read() == open(whole, 'rb').read()


# ------------------------------------------------------------------------------- 8. command line
def test_command_line_select_and_merge(s1, emon_amon):
    d, a, b, va, vb = emon_amon
    done = s1.main(['select', '-i', os.path.join(d, 'emon.nc'), '-o', os.path.join(d, 'cli_{}.nc'), '-v', 'ta', '-l', '85000,25000',
                    '-b', '-73,37,-42,34', '--max_records', '5'])
    assert done == [os.path.join(d, 'cli_ta.nc')]
    ra, _, _ = read_raw(a)
    rs, _, _ = read_raw(done[0])
    assert np.array_equal(words(rs['ta'][0]), words(ra['ta'][0])[:, [1, 4]][:, :, BOX_ROWS][..., BOX_COLS])
    assert np.array_equal(rs['lon'][0], BOX_LON)
    done = s1.main(['merge_levels', os.path.join(d, 'emon.nc'), os.path.join(d, 'amon.nc'), os.path.join(d, 'cli_merged_{}.nc'),
                    '-v', 'ta', '--levels_a', '100000,70000,25000', '--levels_b', '7000,1000'])
    assert done == [os.path.join(d, 'cli_merged_ta.nc')]
    rb, _, _ = read_raw(b)
    rm, _, _ = read_raw(done[0])
    assert np.array_equal(words(rm['ta'][0]), np.concatenate([words(ra['ta'][0])[:, [0, 2, 4]], words(rb['ta'][0])[:, [0, 2]]], axis=1))
    done = s1.main(['climatology', '-i', a, '-o', os.path.join(d, 'cli_clim.nc'), '-v', 'ta', '-m', 'ymonmean', '-b', '-73,37,-42,34'])
    direct = s1.climatology_files([a], os.path.join(d, 'direct_clim.nc'), 'ta', 'ymonmean', box=BOX)
    assert open(done[0], 'rb').read() == open(direct, 'rb').read()
