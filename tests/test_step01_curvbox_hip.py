"""GPU checks of step_01's lon-lat box on curvilinear grids: the marker kernel behind `pgw_box_mark_2d` against the numpy
statement of tests/curvbox_cases.py (flags and count must be EQUAL), and the layers above it in
pgw4era5_amd/step_01_extract_deltas.py - curvilinear_box, select, select_file, climatology_files(box=...), the command line
- against the numpy index statement on unsigned views or on the bytes of a file, and the chain into step_02's ocean
interpolation.  test_step01_curvbox_host.py asserts on the CPU that the shared cases select something non-trivial."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curvbox_cases as C                                                             # noqa: E402

pytestmark = pytest.mark.gpu

PGW_ERR_ARG = 2
GUARD = np.int32(0x5A5A5A5A)
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


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


class Marked:
    """The three outputs of pgw_box_mark_2d in one device buffer of int32 words with guard words around each:
    G G | n_inside (2 words, 8-byte aligned) | G G | row_any (nj) | G | col_any (ni) | G."""

    def __init__(self, ctx, s1, nj, ni):
        self.ctx, self.nj, self.ni = ctx, nj, ni
        self.buf = to_dev(ctx, s1, np.full(8 + nj + ni, GUARD, dtype=np.int32))
        self.p_n, self.p_row, self.p_col = self.buf.ptr + 8, self.buf.ptr + 24, self.buf.ptr + 4 * (7 + nj)

    def read(self):
        w = self.buf.numpy()
        nj, ni = self.nj, self.ni
        guards = np.concatenate([w[0:2], w[4:6], w[6 + nj:7 + nj], w[7 + nj + ni:]])
        return w[6:6 + nj], w[7 + nj:7 + nj + ni], int(w[2:4].view(np.int64)[0]), guards, w


def mark(ctx, s1, lat, lon, box, out=None, dtype_tag=None, nj=None, ni=None, p_lat=0, p_lon=0):
    """One pgw_box_mark_2d call -> (status, message, Marked)."""
    from pgw4era5_amd.device import dtype_tag as tag_of
    d_lat, d_lon = to_dev(ctx, s1, lat), to_dev(ctx, s1, lon)
    out = Marked(ctx, s1, *lat.shape) if out is None else out
    rc = ctx.lib.pgw_box_mark_2d(ctx.handle, tag_of(lat.dtype) if dtype_tag is None else dtype_tag,
                                 lat.shape[0] if nj is None else nj, lat.shape[1] if ni is None else ni,
                                 d_lat.ptr if p_lat == 0 else p_lat, d_lon.ptr if p_lon == 0 else p_lon,
                                 *[float(b) for b in box], out.p_row, out.p_col, out.p_n)
    ctx.sync()
    return rc, (ctx.lib.pgw_last_error(ctx.handle) or b'').decode(), out


def check_marks(ctx, s1, lat, lon, box):
    rc, msg, out = mark(ctx, s1, lat, lon, box)
    assert rc == 0, msg
    row_any, col_any, n, guards, _ = out.read()
    want_row, want_col, want_n = C.flags_ref(lat, lon, box)
    assert np.array_equal(row_any, want_row) and np.array_equal(col_any, want_col) and n == want_n, (lat.shape, lat.dtype, box)
    assert np.all(guards == GUARD)
    return n


# ------------------------------------------------------------------------------- 1. the kernel against the statement
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', C.KERNEL_SHAPES)
def test_mark_vs_statement(ctx, s1, shape, dtype):
    nj, ni = shape
    lat, lon = C.scatter_grid(nj, ni, dtype, seed=1000 * nj + ni)
    for box in C.BOXES:
        check_marks(ctx, s1, lat, lon, box)
    ok = np.isfinite(lat) & np.isfinite(lon)
    assert check_marks(ctx, s1, lat, lon, C.GLOBAL_BOX) == int(ok.sum())           # the whole circle: every finite cell
    if nj * ni >= 64:
        assert 0 < check_marks(ctx, s1, lat, lon, C.REF_BOX) < ok.sum()
    # the smooth ocean grid of that shape (the shapes with a single column need ni >= 1 only), NaN / inf sprinkled in
    glat, glon = C.ocean_grid(nj, ni, dtype)
    for box in C.BOXES:
        check_marks(ctx, s1, glat, glon, box)
        check_marks(ctx, s1, *C.sprinkle(glat, glon, seed=ni), box)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_mark_edges(ctx, s1, dtype):
    lat, lon, table = C.edge_grid(dtype)
    rc, msg, out = mark(ctx, s1, lat, lon, C.REF_BOX)
    assert rc == 0, msg
    row_any, col_any, n, guards, _ = out.read()
    want = C.edge_expectation(table)
    ins = np.zeros(lat.size, dtype=bool)
    ins[[k for k, v in want.items() if v]] = True
    ins = ins.reshape(lat.shape)
    assert n == ins.sum() == sum(want.values())
    assert np.array_equal(row_any, ins.any(axis=1).astype(np.int32)) and np.array_equal(col_any, ins.any(axis=0).astype(np.int32))
    # cell by cell: a grid of one cell per table entry
    for k, edge, kind in table:
        one = (lat.reshape(-1)[k:k + 1].reshape(1, 1).copy(), lon.reshape(-1)[k:k + 1].reshape(1, 1).copy())
        assert check_marks(ctx, s1, one[0], one[1], C.REF_BOX) == (1 if want[k] else 0), (edge, kind)
    check_marks(ctx, s1, lat, lon, (-73.0, 37.0, 34.0, -42.0))                  # lat1 > lat2


def test_mark_all_outside(ctx, s1):
    lat, lon = C.ocean_grid(17, 257)
    lat = np.full_like(lat, -80.0)
    rc, msg, out = mark(ctx, s1, lat, lon, C.REF_BOX)
    row_any, col_any, n, guards, _ = out.read()
    assert rc == 0 and n == 0 and not row_any.any() and not col_any.any() and np.all(guards == GUARD)
    with pytest.raises(ValueError, match='no cell lies within'):
        s1.curvilinear_box(lat, lon, C.REF_BOX)


def test_mark_argument_errors(ctx, s1):
    lat, lon = C.ocean_grid(5, 130)
    out = Marked(ctx, s1, 5, 130)
    before = out.read()[4].copy()
    nan = float('nan')
    bad = [(dict(nj=0), 'positive'), (dict(ni=0), 'positive'), (dict(nj=-1), 'positive'), (dict(p_lat=None), 'null pointer'),
           (dict(p_lon=None), 'null pointer'), (dict(dtype_tag=2), 'dtype'), (dict(dtype_tag=-1), 'dtype'),
           (dict(box=(nan, 37.0, -42.0, 34.0)), 'NaN'), (dict(box=(-73.0, nan, -42.0, 34.0)), 'NaN'),
           (dict(box=(-73.0, 37.0, nan, 34.0)), 'NaN'), (dict(box=(-73.0, 37.0, -42.0, nan)), 'NaN'),
           (dict(box=(37.0, -73.0, -42.0, 34.0)), 'lon1 < lon2'), (dict(box=(5.0, 5.0, -42.0, 34.0)), 'lon1 < lon2'),
           (dict(box=(0.0, 360.5, -42.0, 34.0)), 'lon2 - lon1 <= 360')]
    for kw, text in bad:
        kw = dict(kw)
        box = kw.pop('box', C.REF_BOX)
        rc, msg, _ = mark(ctx, s1, lat, lon, box, out=out, **kw)
        assert rc == PGW_ERR_ARG and msg.startswith('pgw_box_mark_2d: ') and text in msg, (kw, box, rc, msg)
        assert np.array_equal(out.read()[4], before), (kw, box)                  # all outputs untouched
    # a null output pointer
    d_lat, d_lon = to_dev(ctx, s1, lat), to_dev(ctx, s1, lon)
    for k in range(3):
        ptrs = [out.p_row, out.p_col, out.p_n]
        ptrs[k] = None
        rc = ctx.lib.pgw_box_mark_2d(ctx.handle, 1, 5, 130, d_lat.ptr, d_lon.ptr, -73.0, 37.0, -42.0, 34.0, *ptrs)
        ctx.sync()
        assert rc == PGW_ERR_ARG and np.array_equal(out.read()[4], before)
    # and the good call on the same buffer
    rc, msg, _ = mark(ctx, s1, lat, lon, C.REF_BOX, out=out)
    row_any, col_any, n, guards, _ = out.read()
    assert rc == 0 and n == C.flags_ref(lat, lon, C.REF_BOX)[2] > 0 and np.all(guards == GUARD)


# ------------------------------------------------------------------------------- curvilinear_box
def test_curvilinear_box(s1):
    for name, (lat, lon, cyc) in C.grid_kinds(40, 60).items():
        for box in C.BOXES:
            for dtype in (np.float64, np.float32):
                la, lo = lat.astype(dtype), lon.astype(dtype)
                for cyclic in ('auto', True, False):
                    got = s1.curvilinear_box(la, lo, box, cyclic=cyclic)
                    assert got == C.box_ref(la, lo, box, cyclic) and all(type(g) is int for g in got), (name, box, dtype, cyclic)
    lat, lon = C.ocean_grid(40, 60)
    assert s1.curvilinear_box(lat, lon, C.REF_BOX)[2:4] == (47, 19)            # columns 47 .. 59, 0 .. 5: across the seam
    assert s1.curvilinear_box(lat, lon, C.REF_BOX, cyclic=False)[2:4] == (0, 60)
    la, lo = C.regional_grid()
    assert s1.curvilinear_box(la, lo, (10.0, 30.0, 35.0, 50.0)) == C.box_ref(la, lo, (10.0, 30.0, 35.0, 50.0), False)
    la, lo, _ = C.edge_grid(np.float32)
    assert s1.curvilinear_box(la, lo, C.REF_BOX) == C.box_ref(la, lo, C.REF_BOX)


# ------------------------------------------------------------------------------- 2. select
def bit_patterns(shape, elem_bytes, seed):
    rng = np.random.default_rng(seed)
    u = UINT[elem_bytes]
    x = rng.integers(0, 2**(8 * elem_bytes), size=shape, dtype=u, endpoint=False)
    special = {2: [0xFFFF, 0x8000, 0x7FFF], 4: [0xFFFFFFFF, 0x7FC00001, 0x7F800001, 0x7E967699],
               8: [0xFFFFFFFFFFFFFFFF, 0x7FF8000000000001, 0x7FF0000000000001, 0x479E17B84357691B]}[elem_bytes]
    flat = x.reshape(-1)
    where = rng.random(flat.shape) < 0.2
    flat[where] = rng.choice(np.array(special, dtype=u), size=int(where.sum()))
    return x


SELECT_GRIDS = {'seam': (lambda: C.ocean_grid(40, 60), C.REF_BOX), 'plain': (lambda: C.ocean_grid(40, 60), C.ASIA_BOX),
                'halo': (lambda: C.grid_kinds(12, 65)['halo'][:2], C.REF_BOX), 'regional': (C.regional_grid, (10.0, 30.0, 35.0, 50.0))}


@pytest.mark.parametrize('grid', sorted(SELECT_GRIDS))
@pytest.mark.parametrize('elem_bytes', [2, 4, 8])
def test_select_arrays(ctx, s1, elem_bytes, grid):
    from pgw4era5_amd import ncio
    make, box = SELECT_GRIDS[grid]
    lat, lon = make()
    nj, ni = lat.shape
    win = C.box_ref(lat, lon, box)
    assert win[4] >= 2 and (win[1] < nj or win[3] < ni)
    plev = np.array([100000.0, 85000.0, 50000.0])
    for has_lev in (False, True):
        shape = (2, 3, nj, ni) if has_lev else (3, nj, ni)
        src = bit_patterns(shape, elem_bytes, seed=elem_bytes + nj)
        want = C.index_ref(src, *win[:4])
        kw = dict(plev=plev) if has_lev else {}
        got = s1.select(src, box=box, lat=lat, lon=lon, **kw)                   # numpy in, numpy out
        assert got.dtype == src.dtype and np.array_equal(got, want)
        if has_lev:                                                             # with a level list on top
            got = s1.select(src, levels=[50000, 100000], box=box, lat=lat, lon=lon, plev=plev)
            assert np.array_equal(got, want[:, [0, 2]])
        d = s1.select(to_dev(ctx, s1, src), box=box, lat=lat, lon=lon, **kw)    # DeviceArray in, DeviceArray out
        assert d.shape == want.shape and np.array_equal(d.numpy(), want)
        for cyclic in (True, False):                                            # the window forced either way
            w = C.box_ref(lat, lon, box, cyclic)
            got = s1.select(src, box=box, lat=lat, lon=lon, cyclic=cyclic, **kw)
            assert np.array_equal(got, C.index_ref(src, *w[:4]))
        # ncio.Field with the 2-D coordinates among its coords: the coordinates come back cut, bits kept
        dims = (('time', 'plev') if has_lev else ('time',)) + ('j', 'i')
        coords = {'latitude': lat, 'longitude': lon, 'j': np.arange(nj), 'i': np.arange(ni)}
        if has_lev:
            coords['plev'] = plev
        f = ncio.Field(src, dims, coords, {'units': 'K'}, 'tos')
        out = s1.select(f, box=box)
        assert isinstance(out, ncio.Field) and out.dims == dims and out.attrs == {'units': 'K'} and out.name == 'tos'
        assert out.values.dtype == src.dtype and np.array_equal(out.values, want)
        assert np.array_equal(C.words(out.coords['latitude']), C.words(C.index_ref(lat, *win[:4])))
        assert np.array_equal(C.words(out.coords['longitude']), C.words(C.index_ref(lon, *win[:4])))
        assert np.array_equal(out.coords['j'], np.arange(win[0], win[0] + win[1]))
        assert np.array_equal(out.coords['i'], (win[2] + np.arange(win[3])) % ni)
    f32 = bit_patterns((2, nj, ni), 4, seed=9).view(np.float32)                 # a float view: NaN payloads go through
    out = s1.select(f32, box=box, lat=lat.astype(np.float32), lon=lon.astype(np.float32))
    w32 = C.box_ref(lat.astype(np.float32), lon.astype(np.float32), box)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), C.index_ref(f32.view(np.uint32), *w32[:4]))


# ------------------------------------------------------------------------------- 3. select_file
def check_cut_file(inp, out, var, win, jdim, idim):
    """Every variable of `out` is the variable of `inp` cut along the grid dimensions, as raw file words; attributes,
    dimensions' names, global attributes and the record dimension are carried over."""
    a, ga, reca = C.read_raw(inp)
    b, gb, recb = C.read_raw(out)
    assert list(a) == list(b) and C.same_attrs(ga, gb) and reca == recb == ['time']
    n_cut = 0
    for name in a:
        data, dims, attrs = a[name]
        assert b[name][1] == dims and C.same_attrs(attrs, b[name][2]) and b[name][0].dtype == data.dtype, name
        jax = dims.index(jdim) if jdim in dims else None
        iax = dims.index(idim) if idim in dims else None
        want = C.words(data) if data.ndim else data
        if jax is not None or iax is not None:
            want = C.index_ref(want, *win[:4], jax=jax, iax=iax)
            n_cut += 1
        got = C.words(b[name][0]) if data.ndim else b[name][0]
        assert got.shape == want.shape and np.array_equal(got, want), name
    return a, b, n_cut


@pytest.mark.parametrize('box', ['seam', 'plain'])
def test_select_file_ocean(s1, tmp_path, box):
    box = {'seam': C.REF_BOX, 'plain': C.ASIA_BOX}[box]
    inp = str(tmp_path / 'tos.nc')
    info = C.write_ocean_file(inp)
    win = C.box_ref(info['lat'], info['lon'], box)
    assert win[4] >= 2 and win[3] <= 30
    out = s1.select_file(inp, str(tmp_path / 'out.nc'), 'tos', box=box)
    a, b, n_cut = check_cut_file(inp, out, 'tos', win, 'j', 'i')
    assert n_cut == 8                                              # tos, j, i, latitude, longitude, two vertices_*, areacello
    assert b['tos'][0].shape == (12, win[1], win[3]) and b['vertices_longitude'][0].shape == (win[1], win[3], 4)
    assert b['tos'][2]['_FillValue'] == np.float32(1.0e20)
    fill = b['tos'][0] == np.float32(1.0e20)
    assert fill.any() or not C.index_ref(info['land'], *win[:4]).any()
    assert not fill.all()
    # the coordinates keep their bits: no 360 k shift, whichever side of the seam
    assert np.array_equal(C.words(b['longitude'][0]), C.words(C.index_ref(a['longitude'][0], *win[:4])))
    assert b['longitude'][0].min() >= 0.0
    # independent of max_records; cyclic forced; the identity box gives the file's bytes back
    one = s1.select_file(inp, str(tmp_path / 'one.nc'), 'tos', box=box, max_records=1)
    assert open(one, 'rb').read() == open(out, 'rb').read()
    plain = s1.select_file(inp, str(tmp_path / 'plain.nc'), 'tos', box=box, cyclic=False)
    check_cut_file(inp, plain, 'tos', C.box_ref(info['lat'], info['lon'], box, False), 'j', 'i')
    ident = s1.select_file(inp, str(tmp_path / 'ident.nc'), 'tos', box=C.GLOBAL_BOX)
    c, _, _ = C.read_raw(ident)
    for name in a:
        assert c[name][0].tobytes() == a[name][0].tobytes(), name
    # a variable without 2-D coordinates on its last two dimensions behaves as before
    with pytest.raises(ValueError, match='must end in'):
        s1.select_file(inp, str(tmp_path / 'x.nc'), 'vertices_latitude', box=box)
    with pytest.raises(ValueError, match='no cell lies within'):
        s1.select_file(inp, str(tmp_path / 'x.nc'), 'tos', box=(0.0, 10.0, -90.0, -89.9))


def test_select_file_regional(s1, tmp_path):
    inp = str(tmp_path / 'ta.nc')
    info = C.write_regional_file(inp)
    box = (10.0, 30.0, 35.0, 50.0)
    win = C.box_ref(info['lat'], info['lon'], box)
    assert win == C.box_ref(info['lat'], info['lon'], box, False) and win[4] >= 2
    assert win[1] < info['lat'].shape[0] and win[3] < info['lat'].shape[1]
    out = s1.select_file(inp, str(tmp_path / 'out.nc'), 'ta', box=box)
    a, b, n_cut = check_cut_file(inp, out, 'ta', win, 'rlat', 'rlon')
    assert n_cut == 5 and b['ta'][0].shape == (3, 3, win[1], win[3])            # ta, rlat, rlon, lat, lon
    one = s1.select_file(inp, str(tmp_path / 'one.nc'), 'ta', box=box, max_records=1)
    assert open(one, 'rb').read() == open(out, 'rb').read()
    lev = s1.select_file(inp, str(tmp_path / 'lev.nc'), 'ta', levels=[50000, 100000], box=box)
    c, _, _ = C.read_raw(lev)
    assert np.array_equal(C.words(c['ta'][0]), C.words(b['ta'][0])[:, [0, 2]]) and c['plev'][0].tolist() == [100000.0, 50000.0]


# ------------------------------------------------------------------------------- 4. climatology with a box
def test_climatology_with_box(s1, tmp_path):
    paths, cut_paths = [], []
    for y in range(2):
        p = str(tmp_path / ('y%d.nc' % y))
        info = C.write_ocean_file(p, times=C.MONTHS + 365.0 * y, seed=y)
        paths.append(p)
        cut_paths.append(s1.select_file(p, str(tmp_path / ('y%d_box.nc' % y)), 'tos', box=C.REF_BOX))
    boxed = s1.climatology_files(paths, str(tmp_path / 'clim_box.nc'), 'tos', 'ymonmean', box=C.REF_BOX)
    of_cut = s1.climatology_files(cut_paths, str(tmp_path / 'clim_of_cut.nc'), 'tos', 'ymonmean')
    whole = s1.climatology_files(paths, str(tmp_path / 'clim.nc'), 'tos', 'ymonmean')
    assert open(boxed, 'rb').read() == open(of_cut, 'rb').read()
    win = C.box_ref(info['lat'], info['lon'], C.REF_BOX)
    rb, _, _ = C.read_raw(boxed)
    rw, _, _ = C.read_raw(whole)
    assert rb['tos'][0].shape == (12, win[1], win[3]) and win[3] == 19
    assert np.array_equal(C.words(rb['tos'][0]), C.index_ref(C.words(rw['tos'][0]), *win[:4]))
    assert np.array_equal(C.words(rb['latitude'][0]), C.index_ref(C.words(rw['latitude'][0]), *win[:4]))
    assert np.any(rb['tos'][0] != np.float32(1.0e20))
    again = s1.climatology_files(paths, str(tmp_path / 'clim_box1.nc'), 'tos', 'ymonmean', box=C.REF_BOX, max_records=1)
    assert open(again, 'rb').read() == open(boxed, 'rb').read()
    plain = s1.climatology_files(paths, str(tmp_path / 'clim_plain.nc'), 'tos', 'ymonmean', box=C.REF_BOX, cyclic=False)
    rp, _, _ = C.read_raw(plain)
    assert rp['tos'][0].shape == (12, win[1], 60)


# ------------------------------------------------------------------------------- 5. command line
def test_command_line(s1, tmp_path):
    inp = str(tmp_path / 'tos.nc')
    info = C.write_ocean_file(inp)
    for flag, cyclic in (('auto', 'auto'), ('yes', True), ('no', False)):
        done = s1.main(['select', '-i', str(tmp_path / '{}.nc'), '-o', str(tmp_path / ('cli_%s_{}.nc' % flag)), '-v', 'tos',
                        '-b', '-73,37,-42,34', '--cyclic', flag])
        direct = s1.select_file(inp, str(tmp_path / 'direct.nc'), 'tos', box=C.REF_BOX, cyclic=cyclic)
        assert done == [str(tmp_path / ('cli_%s_tos.nc' % flag))] and open(done[0], 'rb').read() == open(direct, 'rb').read()
        done = s1.main(['climatology', '-i', inp, '-o', str(tmp_path / ('clim_%s.nc' % flag)), '-v', 'tos', '-m', 'ymonmean',
                        '-b', '-73,37,-42,34', '--cyclic', flag])
        direct = s1.climatology_files([inp], str(tmp_path / 'direct_clim.nc'), 'tos', 'ymonmean', box=C.REF_BOX, cyclic=cyclic)
        assert open(done[0], 'rb').read() == open(direct, 'rb').read()
    r, _, _ = C.read_raw(str(tmp_path / 'cli_auto_tos.nc'))
    assert r['tos'][0].shape[2] == 19
    r, _, _ = C.read_raw(str(tmp_path / 'cli_no_tos.nc'))
    assert r['tos'][0].shape[2] == 60
    done = s1.main(['select', '-i', inp, '-o', str(tmp_path / 'nocyc.nc'), '-v', 'tos', '-b', '20,120,-30,60'])     # the default
    assert open(done[0], 'rb').read() == open(s1.select_file(inp, str(tmp_path / 'd2.nc'), 'tos', box=C.ASIA_BOX), 'rb').read()


# ------------------------------------------------------------------------------- 6. the chain into step_02
def test_chain_into_step_02(s1, tmp_path):
    """step_02 `regridding -v tos` from the cut tos_delta.nc and from the uncut one onto a small regular target that lies
    30 degrees inside the box 20,120,-30,60 on every side.  step_02 runs with the kernel radius of settings (1000 km), in
    the interpolation's planar metres (x: the meridian arc, y: longitude times the cosine of the point's OWN latitude):
    a point beyond lon 120 within 1000 km in x of the target (30 N, 90 E) lies at 39 N or south of it, where y is 120 *
    cos(39) = 93 against the target's 78 degrees of arc - 1700 km away; the other three sides are further.  So both sources
    give every target the same contributing points, in another order (the cells of the cloud differ).
    |a - b| <= 4 n eps max|v|: the reordering bound of a weighted mean of at most n terms (n: the points of the uncut
    file)."""
    from pgw4era5_amd import ncio, settings, step_02_preproc_deltas as s2
    F = ncio.Field
    assert settings.nan_interp_kernel_radius <= 1000000
    whole, cut = tmp_path / 'whole', tmp_path / 'cut'
    whole.mkdir(); cut.mkdir()
    nj, ni = 90, 180
    for base, seed in (('tos_delta.nc', 0), ('tos_historical.nc', 1)):
        info = C.write_ocean_file(str(whole / base), nj=nj, ni=ni, dtype=np.float64, seed=seed)
        s1.select_file(str(whole / base), str(cut / base), 'tos', box=C.ASIA_BOX)
        if base == 'tos_delta.nc':
            delta = info
    win = C.box_ref(delta['lat'], delta['lon'], C.ASIA_BOX)
    assert win[4] >= 2 and win[1] < nj and win[3] < ni
    tlat, tlon = np.linspace(0.0, 30.0, 11), np.linspace(50.0, 90.0, 13)
    lon1, lon2, lat1, lat2 = C.ASIA_BOX
    assert tlat.min() - lat1 >= 20 and lat2 - tlat.max() >= 20 and tlon.min() - lon1 >= 20 and lon2 - tlon.max() >= 20
    era = ncio.Dataset()
    era['lat'] = F(tlat, ('lat',)); era['lon'] = F(tlon, ('lon',))
    era['FR_LAND'] = F(np.zeros((1, 11, 13)), ('time', 'lat', 'lon'))
    era['time'] = F(np.array([0.0]), ('time',))
    ncio.to_netcdf(era, str(tmp_path / 'era.nc'))
    res = {}
    for name, d in (('whole', whole), ('cut', cut)):
        out = tmp_path / ('out_' + name)
        s2.main(['regridding', '-i', str(d), '-o', str(out), '-e', str(tmp_path / 'era.nc'), '-v', 'tos'])
        res[name] = np.asarray(ncio.open_dataset(str(out / 'tos_delta.nc'))['tos'].values, dtype=np.float64)
    a, b = res['whole'], res['cut']
    assert a.shape == b.shape == (12, 11, 13)
    fin = np.isfinite(a) & np.isfinite(b)
    assert fin.sum() > a.size / 2 and np.array_equal(np.isnan(a), np.isnan(b))
    v = delta['values'][delta['values'] != C.FILL]
    bound = 4 * (nj * ni) * np.finfo(np.float64).eps * np.max(np.abs(v))
    err = np.max(np.abs(a[fin] - b[fin]))
    print('chain: max |a - b| = %.3e, bound %.3e, %d of %d targets finite' % (err, bound, fin.sum(), a.size))
    assert err <= bound
