"""step_03 on climate deltas that lie on the GCM's grid with every column of the file a target of its own
(settings.delta_grid = 'source_points'), the winds rotated onto a rotated-pole file's directions (--rotate_winds), and the
points plan behind it, on the GPU.  The reference of every comparison is code that was there before: `functions.regrid_points`
/ `regrid_points_wind` / `regrid_lat_lon_wind` on the whole array with the cast made on the host, `RegridPlan.apply` for a mesh
handed over as points, `step_02 regridding [--rotate_winds]` into files with step_03 on those files, `--delta_grid source` on
mesh files.  Every comparison is for equal bits or bytes; the cases and their conditions are tests/source_points_cases.py's
(asserted on the CPU by tests/test_source_points_host.py)."""
import ctypes as C
import datetime as dt
import os

import numpy as np
import pytest

import points_file_cases as P
import source_delta_cases as K
import source_points_cases as Q
import wind_rotation_cases as W

pytestmark = pytest.mark.gpu

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
PGW_OK, PGW_ERR_ARG = 0, 2
FILL = -777.0                                 # what guard words and output slots hold before a call
DT = {'f32': np.dtype('float32'), 'f64': np.dtype('float64')}
TABLES = 'lat_lo lat_hi lat_dx lat_Dx lon_lo lon_hi lon_dx lon_Dx oob'.split()
MODES = ['float64 files, float32 deltas', 'float32 files (reference), float64 deltas']
# rotation runs on the two rotated files only: a cell list has no grid directions
RUNS = [(name, rotate) for name in P.FILES for rotate in (False, True) if not rotate or P.FILES[name][0] == 'rotated']
RUN_IDS = ['%s%s' % (n, ', rotated winds' if r else '') for n, r in RUNS]


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    return default_context()


@pytest.fixture
def clean(monkeypatch):
    """No DeltaSet of an earlier test; PGW_DELTA_GRID, PGW_ROTATE_WINDS and PGW_DELTA_RESIDENT as found afterwards; quiet."""
    from pgw4era5_amd import settings as S, step_03_apply_to_era as s3
    P.forget(s3)
    for name in ('PGW_DELTA_GRID', 'PGW_ROTATE_WINDS', 'PGW_DELTA_RESIDENT'):       # registered: whatever a test leaves is undone
        monkeypatch.setenv(name, '0')
        monkeypatch.delenv(name)
    monkeypatch.setattr(S, 'i_debug', -1)
    yield monkeypatch
    P.forget(s3)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, ref, cast):
    """Equal bits; where a cast lies between the two, a NaN matches a NaN (its payload is not pinned by a cast)."""
    same = _bits(got) == _bits(ref)
    if cast:
        same |= np.isnan(got) & np.isnan(ref)
    return same


class Slot:
    """An output slot of `n` elements inside one allocation: GUARD words, `offset` more, the slot, GUARD words - all FILL."""

    def __init__(self, ctx, nmax, dtype):
        self.ctx, self.dtype = ctx, np.dtype(dtype)
        self.host = np.full(Q.GUARD + max(Q.OFFSETS) + nmax + Q.GUARD, FILL, dtype=self.dtype)
        self.buf = ctx.to_device(self.host)

    def take(self, shape, offset):
        from pgw4era5_amd.device import DeviceArray
        self.buf.copy_from(self.host)
        self.at, self.n = Q.GUARD + offset, int(np.prod(shape))
        return DeviceArray(self.ctx, shape, self.dtype, ptr=self.buf.ptr + self.at * self.dtype.itemsize, owner=self.buf)

    def read(self, shape):
        """The slot's values, after the words around it were found unchanged."""
        whole = self.buf.numpy()
        around = np.concatenate([whole[:self.at], whole[self.at + self.n:]])
        np.testing.assert_array_equal(_bits(around), _bits(np.full(around.shape, FILL, dtype=self.dtype)), err_msg='guard words')
        return whole[self.at:self.at + self.n].reshape(shape)


# ------------------------------------------------------------------ 1. the plan against the per-call entries
@pytest.mark.parametrize('nan', [False, True], ids=['finite', 'nan'])
@pytest.mark.parametrize('index', range(len(K.grid_pairs())), ids=K.pair_ids())
def test_points_plan_is_the_per_call_entries_bit_for_bit(ctx, index, nan):
    """Per source grid and target count one plan with a pole, applied with 40, 3 and 1 planes, float32 / float64 sources into
    float32 / float64 slots 0, 1 and 2 elements behind a 16-byte boundary: `apply` holds the bits of functions.regrid_points,
    `apply_wind` those of functions.regrid_points_wind, cast on the host where the slot's type differs; the words around the
    slots stay as they were."""
    from pgw4era5_amd import functions as F
    pair = K.grid_pairs()[index]
    name, slat, slon = pair[:3]
    for j, n in enumerate(Q.NPOINTS):
        lat, lon = Q.targets(pair, n)
        pole = Q.pole_of(index + j)
        cos, sin = F.wind_rotation(lat, lon, *pole)
        plan = F.PointsPlan(slat, slon, lat, lon, max(Q.NFIELDS), pole=pole, ctx=ctx)
        slots = {k: [Slot(ctx, max(Q.NFIELDS) * n, d) for _ in range(2)] for k, d in DT.items()}
        tb = Q.point_tables(pair, lat, lon) if nan else None
        try:
            for nfield in Q.NFIELDS:
                for sk, sdt in DT.items():
                    field = K.plan_field(name, nfield, len(slat), len(slon), sdt, nan=tb)
                    other = np.ascontiguousarray(field[::-1] * sdt.type(0.5) + sdt.type(3.0))       # the second wind component
                    want = np.asarray(F.regrid_points(field, slat, slon, lat, lon))                 # pgw_regrid_points, whole array
                    want_u, want_v = (np.asarray(x) for x in F.regrid_points_wind(field, other, slat, slon, lat, lon, cos, sin))
                    assert want.dtype == sdt and want.shape == (nfield, n) and want_u.dtype == sdt and want_v.shape == (nfield, n)
                    assert np.isnan(want).any() == nan and (nfield == 1 or np.isfinite(want[1]).all())
                    src, src_o = ctx.to_device(field), ctx.to_device(other)
                    for ok, odt in DT.items():
                        ref, ref_u, ref_v = want.astype(odt), want_u.astype(odt), want_v.astype(odt)      # the casts the host makes today
                        for offset in Q.OFFSETS:
                            tag = '%s n %d %s->%s nfield %d offset %d' % (name, n, sk, ok, nfield, offset)
                            out = slots[ok][0].take(ref.shape, offset)
                            assert out.ptr % odt.itemsize == 0 and (out.ptr % 16 == 0) == (offset * odt.itemsize % 16 == 0)
                            plan.apply(src, out)
                            assert _same(slots[ok][0].read(ref.shape), ref, sk != ok).all(), 'apply ' + tag
                            out_u, out_v = (s.take(ref.shape, offset) for s in slots[ok])
                            plan.apply_wind(src, src_o, out_u, out_v)
                            assert _same(slots[ok][0].read(ref.shape), ref_u, sk != ok).all(), 'apply_wind u ' + tag
                            assert _same(slots[ok][1].read(ref.shape), ref_v, sk != ok).all(), 'apply_wind v ' + tag
                    src.free()
                    src_o.free()
        finally:
            plan.free()
            for pair_of_slots in slots.values():
                for s in pair_of_slots:
                    s.buf.free()


@pytest.mark.parametrize('index', range(len(K.grid_pairs())), ids=K.pair_ids())
def test_a_mesh_handed_over_as_points_is_the_regrid_plan(ctx, index):
    """The pair's own mesh target as point-wise targets of the shape (nlat_t, nlon_t): PointsPlan.apply holds the bits
    RegridPlan.apply writes (pgw_regrid_bilinear's), for every dtype pair, NaN corners and NaN pole values included."""
    from pgw4era5_amd import functions as F
    name, slat, slon, tlat, tlon = K.grid_pairs()[index]
    la, lo = np.meshgrid(tlat, tlon, indexing='ij')
    mesh = F.RegridPlan(slat, slon, tlat, tlon, max(Q.NFIELDS), ctx=ctx)
    points = F.PointsPlan(slat, slon, la, lo, max(Q.NFIELDS), ctx=ctx)
    tb = F.regrid_tables(slat, slon, tlat, tlon)
    try:
        assert points.targ_shape == mesh.targ_shape
        for nfield in Q.NFIELDS:
            for sk, sdt in DT.items():
                src = ctx.to_device(K.plan_field(name, nfield, len(slat), len(slon), sdt, nan=tb))
                for ok, odt in DT.items():
                    a, b = (ctx.empty((nfield,) + mesh.targ_shape, odt) for _ in range(2))
                    mesh.apply(src, a)
                    points.apply(src, b)
                    ref, got = a.numpy(), b.numpy()
                    assert np.isnan(ref).any()
                    assert _same(got, ref, sk != ok).all(), '%s %s->%s nfield %d' % (name, sk, ok, nfield)
                    a.free()
                    b.free()
                src.free()
    finally:
        mesh.free()
        points.free()


# ------------------------------------------------------------------ 2. argument errors
def test_points_plan_argument_errors_launch_nothing(ctx):
    """Every PGW_ERR_ARG of create (no plan comes back) and of apply / apply_wind (the slots keep their fill, nothing is timed
    under 'regrid'); the plans then serve good calls - one of them on tables with flagged (oob) targets whose entries are
    unreadable, against pgw_regrid_points / pgw_regrid_points_wind on the same tables."""
    from pgw4era5_amd import _lib, functions as F
    pair = [p for p in K.grid_pairs() if p[0] == '5x8 asc 0..360 poles'][0]
    slat, slon = pair[1:3]
    n = 65
    lat, lon = Q.targets(pair, n)
    tb = Q.point_tables(pair, lat, lon)
    base = {k: np.ascontiguousarray(tb[k]) for k in TABLES}
    assert tb['south_row'] == 0 and tb['north_row'] == 4
    cos, sin = (ctx.to_device(x) for x in F.wind_rotation(lat, lon, *W.POLES[0]))
    made = []

    def create(nlat_s=5, nlon_s=8, ntarg=n, south=0, north=4, max_nfield=3, null=None, no_plan=False, cs=(cos.ptr, sin.ptr), tables=base,
               **edit):
        t = {k: v.copy() for k, v in tables.items()}
        for k, (i, v) in edit.items():
            t[k][i] = v
        p = [None if k == null else t[k].ctypes.data_as(_ip if t[k].dtype == np.int32 else _dp) for k in TABLES]
        h = C.c_void_p(12345)
        rc = ctx.lib.pgw_points_plan_create(ctx.handle, nlat_s, nlon_s, ntarg, *p, south, north, max_nfield, cs[0], cs[1],
                                            None if no_plan else C.byref(h))
        if rc == PGW_OK:
            made.append(h.value)
        else:
            assert no_plan or h.value is None, 'a refused create left a plan behind'
        return rc

    bad = [create(nlat_s=1), create(nlon_s=1), create(ntarg=0), create(max_nfield=0), create(no_plan=True),
           create(south=5), create(north=5), create(south=-1), create(north=-1), create(cs=(cos.ptr, None)), create(cs=(None, sin.ptr)),
           create(cs=(cos.ptr + 4, sin.ptr)), create(lat_lo=(2, -2)), create(lat_hi=(2, 6)), create(lon_lo=(2, -1)), create(lon_hi=(2, 8))]
    bad += [create(null=k) for k in TABLES]
    assert bad == [PGW_ERR_ARG] * len(bad), bad
    with pytest.raises(ValueError, match='pgw_points_plan_create'):
        ctx._check(create(lat_lo=(2, -2)))
    assert made == []
    flag_tb, flag_idx = Q.flagged(tb, n)
    flag_tables = {k: np.ascontiguousarray(flag_tb[k]) for k in TABLES}
    assert create() == PGW_OK and create(cs=(None, None)) == PGW_OK and create(tables=flag_tables) == PGW_OK
    plan, plain, flagged = made
    field = K.plan_field('errors', 3, 5, 8, np.float32)
    other = np.ascontiguousarray(field[::-1] * np.float32(0.5))
    src, src_o = ctx.to_device(field), ctx.to_device(other)
    shape = (3, n)
    slots = [Slot(ctx, int(np.prod(shape)), np.float32) for _ in range(2)]
    out, out_v = (s.take(shape, 0) for s in slots)
    f32, f64 = _lib.PGW_F32, _lib.PGW_F64

    def apply(p=plan, ds=f32, do=f32, nfield=3, s=src.ptr, o=out.ptr):
        return ctx.lib.pgw_points_plan_apply(ctx.handle, p, ds, do, nfield, s, o)

    def wind(p=plan, ds=f32, do=f32, nfield=3, u=src.ptr, v=src_o.ptr, ou=out.ptr, ov=out_v.ptr):
        return ctx.lib.pgw_points_plan_apply_wind(ctx.handle, p, ds, do, nfield, u, v, ou, ov)

    ctx.profile(True)
    ctx.profile_reset()
    try:
        bad = [apply(p=None), apply(ds=7), apply(do=-1), apply(nfield=0), apply(nfield=4), apply(s=None), apply(o=None),
               apply(o=out.ptr + 2), apply(s=src.ptr + 1), apply(do=f64, o=out.ptr + 4), apply(ds=f64, s=src.ptr + 4)]
        bad += [wind(p=None), wind(ds=7), wind(do=-1), wind(nfield=0), wind(nfield=4), wind(u=None), wind(v=None), wind(ou=None),
                wind(ov=None), wind(ov=out_v.ptr + 2), wind(v=src_o.ptr + 1), wind(do=f64, ou=out.ptr + 4), wind(ds=f64, u=src.ptr + 4),
                wind(p=plain)]
        launches = ctx.profile_get('regrid')[0]
        assert bad == [PGW_ERR_ARG] * len(bad), bad
        assert launches == 0
        assert all((s.read(shape) == FILL).all() for s in slots)
        with pytest.raises(ValueError, match='pgw_points_plan_apply'):
            ctx._check(apply(nfield=4))
        with pytest.raises(ValueError, match='cannot rotate'):
            ctx._check(wind(p=plain))
        assert apply() == PGW_OK
        assert ctx.profile_get('regrid')[0] == 1                       # what the 0 above is counted in
    finally:
        ctx.profile(False)
    want = np.asarray(F.regrid_points(field, slat, slon, lat, lon))
    np.testing.assert_array_equal(_bits(slots[0].read(shape)), _bits(want))
    out, out_v = (s.take(shape, 0) for s in slots)
    assert apply(p=plain) == PGW_OK
    np.testing.assert_array_equal(_bits(slots[0].read(shape)), _bits(want))
    want_u, want_v = (np.asarray(x) for x in F.regrid_points_wind(field, other, slat, slon, lat, lon, cos, sin))
    assert wind() == PGW_OK
    np.testing.assert_array_equal(_bits(slots[0].read(shape)), _bits(want_u))
    np.testing.assert_array_equal(_bits(slots[1].read(shape)), _bits(want_v))
    # flagged targets: NaN there, the other targets as without the flags; the per-call entries on the same tables agree
    nanmask = np.zeros(shape, dtype=bool)
    nanmask[:, flag_idx] = True
    p = [flag_tables[k].ctypes.data_as(_ip if flag_tables[k].dtype == np.int32 else _dp) for k in TABLES]
    ref, ref_u, ref_v = (ctx.empty(shape, np.float32) for _ in range(3))
    assert ctx.lib.pgw_regrid_points(ctx.handle, f32, 3, 5, 8, n, src.ptr, *p, 0, 4, ref.ptr) == PGW_OK
    assert ctx.lib.pgw_regrid_points_wind(ctx.handle, f32, 3, 5, 8, n, src.ptr, src_o.ptr, *p, 0, 4, cos.ptr, sin.ptr, ref_u.ptr,
                                          ref_v.ptr) == PGW_OK
    out, out_v = (s.take(shape, 0) for s in slots)
    assert apply(p=flagged) == PGW_OK
    got = slots[0].read(shape)
    np.testing.assert_array_equal(np.isnan(got), nanmask)
    np.testing.assert_array_equal(_bits(got[~nanmask]), _bits(want[~nanmask]))
    W.same_bits(got, ref.numpy())
    assert wind(p=flagged) == PGW_OK
    got_u, got_v = slots[0].read(shape), slots[1].read(shape)
    np.testing.assert_array_equal(np.isnan(got_u), nanmask)
    np.testing.assert_array_equal(_bits(got_v[~nanmask]), _bits(want_v[~nanmask]))
    W.same_bits(got_u, ref_u.numpy())
    W.same_bits(got_v, ref_v.numpy())
    for h in made:
        assert ctx.lib.pgw_points_plan_destroy(ctx.handle, h) == PGW_OK
    assert ctx.lib.pgw_points_plan_destroy(ctx.handle, None) == PGW_OK
    for x in (src, src_o, cos, sin, ref, ref_u, ref_v) + tuple(s.buf for s in slots):
        x.free()


# ------------------------------------------------------------------ 3. records of a DeltaSet over the paired provider
def _write_source_file(path, var, values, times, plev, lat, lon):
    from pgw4era5_amd import ncio
    F = ncio.Field
    ds = ncio.Dataset()
    ds['time'] = F(times, ('time',)); ds['plev'] = F(plev, ('plev',), attrs=dict(units='Pa'))
    ds['lat'] = F(lat, ('lat',)); ds['lon'] = F(lon, ('lon',))
    ds[var] = F(values, ('time', 'plev', 'lat', 'lon'), {'time': times, 'plev': plev})
    ncio.to_netcdf(ds, path)


@pytest.mark.parametrize('dtypes', [('f32', 'f64'), ('f64', 'f32'), ('f32', 'f32')], ids=lambda d: '%s files, %s DeltaSet' % d)
@pytest.mark.parametrize('axis', ['monthly', 'daily'])
def test_wind_records_are_the_rotated_regridded_files(ctx, clean, tmp_path, axis, dtypes):
    """Source 5 x 8, three levels, targets 6 x 6 with 2-D lat / lon: every ua / va record DeltaSet.rec hands out on a forward
    walk - more bracket moves than the window holds, across the year's end and over the dropped leap day - and on a second
    walk that asks for an evicted record again is the record of `regrid_lat_lon_wind` on the whole files, cast on the host.
    No host synchronisation; both caches hold the same records, never more than WINDOW."""
    from pgw4era5_amd import functions as F, ncio, step_03_apply_to_era as s3
    fdt, ddt = DT[dtypes[0]], DT[dtypes[1]]
    times = K.monthly_axis() if axis == 'monthly' else K.daily_axis_with_leap_day()
    _, slat, slon, tlat, tlon = [p for p in K.grid_pairs() if p[0] == '5x8 asc 0..360 poles'][0]
    la, lo = np.meshgrid(tlat, tlon, indexing='ij')
    pole = W.POLES[1]
    plev = np.array([85000.0, 50000.0, 20000.0])
    values = K.record_field(len(times), (3, 5, 8), fdt)
    paths = {v: str(tmp_path / (v + '_delta.nc')) for v in ('ua', 'va')}
    _write_source_file(paths['ua'], 'ua', values, times, plev, slat, slon)
    _write_source_file(paths['va'], 'va', np.ascontiguousarray(values[::-1] * fdt.type(0.5)), times, plev, slat, slon)
    era5 = ncio.Dataset()
    era5['lat'] = ncio.Field(la, ('rlat', 'rlon')); era5['lon'] = ncio.Field(lo, ('rlat', 'rlon'))
    whole = F.regrid_lat_lon_wind(ncio.open_dataset(paths['ua']), ncio.open_dataset(paths['va']), era5, pole)   # what step_02 writes
    want = {v: ds[v].values.astype(ddt) for v, ds in zip(('ua', 'va'), whole)}                     # what the DeltaSet holds today
    assert whole[0]['ua'].values.dtype == fdt and want['ua'].shape == (len(times), 3) + la.shape
    clean.setenv('PGW_DELTA_RESIDENT', '1')
    plan = F.PointsPlan(slat, slon, la, lo, 3, pole=pole, ctx=ctx)
    readers = [ncio.RecordReader(paths[v], v) for v in ('ua', 'va')]
    s3.check_source_wind_files(*readers)
    pair = s3.SourceWindRecords(ctx, readers[0], readers[1], plan)
    dset = s3.DeltaSet(ctx, {'ua': pair, 'va': pair}, times, plev, ddt)
    assert 'ua' in dset and 'va' in dset and dset.dev == {}
    syncs = []
    real_sync = ctx.sync
    try:
        instants = K.walk(axis)
        for k, t in enumerate(instants + [K.revisit(times, instants)] + instants[-2:]):
            ib, ia, _, _, keep = dset.bracket(t, 'ua')
            ctx.sync = lambda: syncs.append(t) or real_sync()
            order = ('ua', 'va') if k % 2 == 0 else ('va', 'ua')
            recs = {v: [dset.rec(v, keep[i]) for i in (ib, ia)] for v in order}
            ctx.sync = real_sync
            assert list(dset._cache['ua']) == list(dset._cache['va']) and len(dset._cache['ua']) <= s3.DeltaSet.WINDOW
            for v in order:
                for r, arr in zip((keep[ib], keep[ia]), recs[v]):
                    assert arr.dtype == ddt and arr.shape == want[v].shape[1:]
                    assert _same(arr.numpy(), want[v][r], fdt != ddt).all(), '%s record %d at %s' % (v, r, t)
        assert syncs == []
    finally:
        ctx.sync = real_sync
        dset.free()


# ------------------------------------------------------------------ 4. step_03 runs: one step against two
def _two_step_deltas(tmp_path, gcm, example, rotate):
    from pgw4era5_amd import step_02_preproc_deltas as s2
    d = str(tmp_path / 'regridded')
    assert len(s2.main(['regridding', '-i', gcm, '-o', d, '-e', example] + (['--rotate_winds'] if rotate else []))) == 22
    return d


def _era_dtypes(clean, mode):
    from pgw4era5_amd import settings as S
    clean.setattr(S, 'f32_file_mode', 'reference')
    return (np.float64, np.float32) if mode.startswith('float64') else (np.float32, np.float64)


def _one_step(clean, rotate):
    clean.setenv('PGW_DELTA_GRID', 'source_points')
    if rotate:
        clean.setenv('PGW_ROTATE_WINDS', 'auto')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,rotate', RUNS, ids=RUN_IDS)
def test_step03_from_source_points_is_the_two_step_run_byte_for_byte(ctx, clean, tmp_path, name, rotate, mode):
    """The point-wise files of points_file_cases (12 levels), deltas on a 12 x 24 source; instants between two records, on a
    record and in early January.  Leg one: `step_02 regridding -e FILE [--rotate_winds]`, then step_03 on its files with the
    records resident and through the host window.  Leg two: delta_grid = 'source_points' [rotate_winds = auto] on the GCM's
    directory.  The same bytes in every output file, the same pass counts and max_err histories."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    era_dtype, delta_dtype = _era_dtypes(clean, mode)
    gcm = P.gcm_files(tmp_path, dtype=delta_dtype)
    _, paths, _ = P.write_files(tmp_path, name, era_dtype, 'points')
    regridded = _two_step_deltas(tmp_path, gcm, paths[0], rotate)
    two = {}
    for r in ('0', '1'):
        clean.setenv('PGW_DELTA_RESIDENT', r)
        two[r] = P.run_files(ctx, paths, str(tmp_path / ('two' + r)), regridded)
        assert s3._DELTASETS and all(d.resident == (r == '1') for d in s3._DELTASETS.values())
        P.forget(s3)
    clean.delenv('PGW_DELTA_RESIDENT')
    _one_step(clean, rotate)
    one = P.run_files(ctx, paths, str(tmp_path / 'one'), gcm)
    (dset,) = s3._DELTASETS.values()
    assert set(dset._src) == set(s3.DeltaSet.VARS_3D) and set(dset.dev) == set(s3.DeltaSet.VARS_2D)
    assert isinstance(dset._src['ua'], s3.SourceWindRecords) == rotate and (dset._src['ua'] is dset._src['va']) == rotate
    for r in ('0', '1'):
        assert one == two[r], 'n_iter / max_err histories'
        assert len(P.same_files(str(tmp_path / 'one'), str(tmp_path / ('two' + r)))) == len(paths)
    assert all(n >= 1 for n, _ in one)


def test_rotation_changes_the_winds_and_nothing_else(ctx, clean, tmp_path):
    """The rotated and the geographic one-step runs differ in U and V alone: the flag is not a no-op on these files."""
    gcm = P.gcm_files(tmp_path, dtype=np.float32)
    _, paths, _ = P.write_files(tmp_path, 'rotated 7x9', np.float64, 'points', instants=P.INSTANTS[:1])
    from pgw4era5_amd import step_03_apply_to_era as s3
    _one_step(clean, False)
    P.run_files(ctx, paths, str(tmp_path / 'geo'), gcm, instants=P.INSTANTS[:1])
    P.forget(s3)
    _one_step(clean, True)
    P.run_files(ctx, paths, str(tmp_path / 'rot'), gcm, instants=P.INSTANTS[:1])
    name = os.path.basename(paths[0])
    a, b = P.variables(str(tmp_path / 'geo' / name)), P.variables(str(tmp_path / 'rot' / name))
    assert sorted(k for k in a if a[k] != b[k]) == ['U', 'V']


# ------------------------------------------------------------------ 5. mesh files: 'source_points' is 'source'
def _mesh_run(tmp_path, era_dtype, delta_dtype):
    from pgw4era5_amd import synthetic
    gcm = str(tmp_path / 'gcm')
    synthetic.write_gcm_files(gcm, nlat=12, nlon=24, plev=K.PLEV, seed=5, ocean=(12, 16))
    K.rewrite(gcm, dtype=delta_dtype)
    era = str(tmp_path / 'era')
    return gcm, era, [synthetic.write_case_files(K.era_case(t, era_dtype), era, str(tmp_path / 'unused')) for t in K.INSTANTS]


@pytest.mark.parametrize('mode', MODES)
def test_on_mesh_files_source_points_gives_the_bytes_of_source(ctx, clean, tmp_path, mode):
    """The global 10 x 10 mesh files of the 'source' tests (both pole rows, 19 delta levels): every column handed over as a
    point gives the output bytes, pass counts and max_err histories of delta_grid = 'source'."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    era_dtype, delta_dtype = _era_dtypes(clean, mode)
    gcm, _, paths = _mesh_run(tmp_path, era_dtype, delta_dtype)
    hist = {}
    for grid in ('source', 'source_points'):
        clean.setenv('PGW_DELTA_GRID', grid)
        hist[grid] = P.run_files(ctx, paths, str(tmp_path / grid), gcm, instants=K.INSTANTS)
        (dset,) = s3._DELTASETS.values()
        assert type(dset._src['ta'].plan).__name__ == {'source': 'RegridPlan', 'source_points': 'PointsPlan'}[grid]
        P.forget(s3)
    assert hist['source'] == hist['source_points'] and all(n >= 1 for n, _ in hist['source'])
    assert len(P.same_files(str(tmp_path / 'source'), str(tmp_path / 'source_points'))) == len(paths)


# ------------------------------------------------------------------ 6. steady state
def test_a_second_file_inside_the_bracket_launches_no_regridding(ctx, clean, tmp_path):
    """Two files an hour apart between the same two records, winds rotated: the first fills the windows, the second adds no
    launch under 'regrid' - no table upload, no rotation angles, no record."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    instants = (P.INSTANTS[0], P.INSTANTS[0] + dt.timedelta(hours=1))
    gcm = P.gcm_files(tmp_path, dtype=np.float32)
    _, paths, _ = P.write_files(tmp_path, 'rotated 11x24', np.float64, 'points', instants=instants)
    _one_step(clean, True)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        P.run_files(ctx, paths[:1], str(tmp_path / 'out'), gcm, instants=instants[:1])
        first = ctx.profile_get('regrid')[0]
        assert first > 0
        P.run_files(ctx, paths[1:], str(tmp_path / 'out'), gcm, instants=instants[1:])
        assert ctx.profile_get('regrid')[0] == first
    finally:
        ctx.profile(False)
    assert len(s3._DELTASETS) == 1


# ------------------------------------------------------------------ 7. the other entry points, all with rotation
def _cli_legs(clean, tmp_path, extra_one=(), extra_two=(), name='rotated 7x9', instants=P.INSTANTS[:2], span=False):
    """The command line on the GCM's directory (`--delta_grid source_points --rotate_winds` + extra_one) and on the files of
    `step_02 regridding --rotate_winds` (extra_two): the output directories hold the same files with the same bytes."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    gcm = P.gcm_files(tmp_path, dtype=np.float32)
    era_dir, paths, _ = P.write_files(tmp_path, name, np.float64, 'points', instants=instants)
    regridded = _two_step_deltas(tmp_path, gcm, paths[0], True)
    if 'interpolate_time' in extra_two:                                 # that mode also reads ps_delta.nc: step_02 has regridded it
        assert os.path.exists(os.path.join(regridded, 'ps_delta.nc')) and os.path.exists(os.path.join(gcm, 'ps_delta.nc'))
    args = ['-i', era_dir, '-H', '1', '-t']
    outs = []
    for leg, d, extra in (('two', regridded, list(extra_two)),
                          ('one', gcm, ['--delta_grid', 'source_points', '--rotate_winds'] + list(extra_one))):
        out = str(tmp_path / leg)
        n = []
        stamps = ['{:%Y%m%d%H}'.format(t) for t in instants]
        for f, l in ([(stamps[0], stamps[-1])] if span else zip(stamps, stamps)):
            n += list(s3._cli(args + ['-o', out, '-d', d, '-f', f, '-l', l] + extra) or [])
        outs.append((out, n))
        P.forget(s3)
        assert 'PGW_DELTA_GRID' not in os.environ and 'PGW_ROTATE_WINDS' not in os.environ
    assert outs[0][1] == outs[1][1]
    return P.same_files(outs[0][0], outs[1][0]), outs[0][1], (era_dir, gcm, regridded, outs)


def test_cli_source_points_two_ranks(clean, tmp_path):
    """`-p 2`: both flags reach the ranks the command line starts; the bytes of the one-rank two-step run."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    instants = (P.INSTANTS[0], P.INSTANTS[0] + dt.timedelta(hours=1))
    names, n, _ = _cli_legs(clean, tmp_path, extra_one=['-p', '2'], extra_two=['-p', '1'], instants=instants, span=True)
    assert len(names) == 2 and len(n) == 2 and all(k >= 1 for k in n)
    assert s3._DELTASETS == {}                                          # the ranks did the work


@pytest.mark.parametrize('debug', ['interpolate_full', 'interpolate_time'])
def test_cli_source_points_debug_mode(clean, tmp_path, debug):
    names, _, _ = _cli_legs(clean, tmp_path, extra_one=['-D', debug], extra_two=['-D', debug])
    assert len(names) == 2 * (7 if debug == 'interpolate_full' else 9)


def test_check_deltas_on_source_points(clean, tmp_path, capsys):
    """check_deltas on the GCM's directory with both flags writes the bytes of check_deltas on step_02's rotated files."""
    from pgw4era5_amd import check_deltas as CD, step_03_apply_to_era as s3
    names, _, (era_dir, gcm, regridded, outs) = _cli_legs(clean, tmp_path, instants=P.INSTANTS[:1])
    stamp = '{:%Y%m%d%H}'.format(P.INSTANTS[0])
    span = ['-f', stamp, '-l', stamp, '-H', '1']
    pgw = outs[0][0]
    CD._cli(['-i', era_dir, '-g', pgw, '-d', regridded, '-o', str(tmp_path / 'chk_two')] + span)
    P.forget(s3)
    CD._cli(['-i', era_dir, '-g', pgw, '-d', gcm, '-o', str(tmp_path / 'chk_one'), '--delta_grid', 'source_points', '--rotate_winds'] + span)
    capsys.readouterr()
    assert 'PGW_DELTA_GRID' not in os.environ and 'PGW_ROTATE_WINDS' not in os.environ
    assert P.same_files(str(tmp_path / 'chk_one'), str(tmp_path / 'chk_two')) == ['deltacheck_' + names[0]]


# ------------------------------------------------------------------ 8. errors before any launch
def test_errors_before_any_launch(ctx, clean, tmp_path):
    """Through the command line: a source that does not cover the targets (the reference's message), --bands, --rotate_winds
    with each wrong mode and on a mesh file: ValueError, nothing timed under 'regrid', no output directory."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    gcm = P.gcm_files(tmp_path, crop=(-60.0, 40.0, 0.0, 360.0))        # the source ends south of the files' columns
    era_dir, paths, _ = P.write_files(tmp_path, 'rotated 7x9', np.float64, 'points', instants=P.INSTANTS[:1])
    mesh_dir, _, _ = P.write_files(tmp_path, 'rotated 7x9', np.float64, 'mesh', layout='mesh', instants=P.INSTANTS[:1])
    out = tmp_path / 'out'
    stamp = '{:%Y%m%d%H}'.format(P.INSTANTS[0])
    args = ['-o', str(out), '-d', gcm, '-f', stamp, '-l', stamp, '-t']
    ctx.profile(True)
    ctx.profile_reset()
    try:
        with pytest.raises(ValueError, match='ERA5 dataset extends further North or South than GCM dataset!'):
            s3._cli(['-i', era_dir] + args + ['--delta_grid', 'source_points'])
        with pytest.raises(ValueError, match='--bands'):
            s3._cli(['-i', era_dir] + args + ['--delta_grid', 'source_points', '--bands'])
        with pytest.raises(ValueError, match='rotate in step_02'):
            s3._cli(['-i', era_dir] + args + ['--delta_grid', 'era5', '--rotate_winds'])
        with pytest.raises(ValueError, match="delta_grid = 'source'"):
            s3._cli(['-i', era_dir] + args + ['--delta_grid', 'source', '--rotate_winds'])
        with pytest.raises(ValueError, match='nothing to rotate'):
            s3._cli(['-i', mesh_dir] + args + ['--delta_grid', 'source_points', '--rotate_winds', '39.25,-162'])
        assert ctx.profile_get('regrid')[0] == 0
    finally:
        ctx.profile(False)
    assert not out.exists()
    assert s3._DELTASETS == {} and 'PGW_DELTA_GRID' not in os.environ and 'PGW_ROTATE_WINDS' not in os.environ
