"""step_03 on ERA5 files with 2-D lat / lon (a rotated-pole file) or a cell list, on the GPU.  The reference of every
comparison is step_03 on a MESH file that holds the same columns and the same deltas - the code path that was there before.
Every comparison is for equal bytes; the cases, their conditions and the helpers are tests/points_file_cases.py's (the
conditions asserted on the CPU by tests/test_step03_points_host.py)."""
import os
import shutil

import numpy as np
import pytest

import points_file_cases as P

pytestmark = pytest.mark.gpu

MODES = ['float64 files, float32 deltas', 'float32 files (reference), float64 deltas', 'float32 files (fast), float64 deltas']
WRITTEN = ('PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE')


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    return default_context()


@pytest.fixture
def clean(monkeypatch):
    """No DeltaSet of an earlier test, PGW_DELTA_GRID and PGW_DELTA_RESIDENT as found afterwards, quiet drivers."""
    from pgw4era5_amd import settings as S, step_03_apply_to_era as s3
    P.forget(s3)
    for name in ('PGW_DELTA_GRID', 'PGW_DELTA_RESIDENT'):
        monkeypatch.setenv(name, '0')
        monkeypatch.delenv(name)
    monkeypatch.setattr(S, 'i_debug', -1)
    yield monkeypatch
    P.forget(s3)


def _mode(clean, mode):
    from pgw4era5_amd import settings as S
    clean.setattr(S, 'f32_file_mode', 'fast' if 'fast' in mode else 'reference')
    return (np.float64, np.float32) if mode.startswith('float64') else (np.float32, np.float64)


# ------------------------------------------------------------------ the mesh run on the same columns
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(P.FILES))
def test_point_files_are_the_mesh_run_on_the_same_columns(ctx, clean, tmp_path, name, mode):
    """The point-wise file with deltas on its layout against a mesh file that holds the same arrays under lat / lon with
    stand-in axes (the cell list: its one-row mesh): the data bytes of every written variable, the pass counts and the
    max_err histories are equal, through the resident records and through the host window; every other variable of the
    output is the input's, byte for byte."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    era_dtype, _ = _mode(clean, mode)
    _, p_paths, p_deltas = P.write_files(tmp_path, name, era_dtype, 'points')
    _, m_paths, m_deltas = P.write_files(tmp_path, name, era_dtype, 'mesh', layout='mesh')
    assert s3.file_layout(p_paths[0]) == {'rotated': ('rlat', 'rlon'), 'cells': ('cell',)}[P.FILES[name][0]]
    assert s3.file_layout(m_paths[0]) == ('lat', 'lon')
    for resident in ('1', '0'):
        clean.setenv('PGW_DELTA_RESIDENT', resident)
        hp = P.run_files(ctx, p_paths, str(tmp_path / ('out_p' + resident)), p_deltas)
        P.forget(s3)
        hm = P.run_files(ctx, m_paths, str(tmp_path / ('out_m' + resident)), m_deltas)
        P.forget(s3)
        assert hp == hm and all(n >= 1 for n, _ in hp), 'n_iter / max_err histories'
        for pp, mp in zip(p_paths, m_paths):
            got = P.variables(os.path.join(str(tmp_path / ('out_p' + resident)), os.path.basename(pp)))
            ref = P.variables(os.path.join(str(tmp_path / ('out_m' + resident)), os.path.basename(mp)))
            inp = P.variables(pp)
            assert list(got) == list(inp)
            for k in got:
                if k in WRITTEN:
                    assert got[k][1:3] == ref[k][1:3], k                    # dtype and data bytes of the mesh run
                    assert got[k][0] == inp[k][0] and got[k][3] == inp[k][3], k
                    assert got[k][2] != inp[k][2] or k == 'FR_SEA_ICE', k
                else:
                    assert got[k] == inp[k], k                              # lat, lon, rlat, rlon, rotated_pole, FIS, ...


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['rotated 7x9', 'cells 65'])
def test_step02_onto_a_point_file_then_step03_is_the_mesh_run_on_the_same_deltas(ctx, clean, tmp_path, name, mode):
    """`step_02 regridding -e POINT_FILE` with all default variables (k_regrid_points, k_gauss_points), then step_03 on the
    point-wise files with the files it wrote: the written variables, pass counts and max_err histories are those of step_03 on
    mesh files that hold the same columns, with the same regridded arrays laid over (lat, lon).  Mixed delta dtypes."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    era_dtype, delta_dtype = _mode(clean, mode)
    gcm = P.gcm_files(tmp_path, dtype=delta_dtype)
    _, p_paths, _ = P.write_files(tmp_path, name, era_dtype, 'points')
    _, m_paths, _ = P.write_files(tmp_path, name, era_dtype, 'mesh', layout='mesh')
    regridded = P.regrid_onto(tmp_path, gcm, p_paths[0])
    nlat, nlon = (1, 65) if name.startswith('cells') else P.FILES[name][1:]
    as_mesh = str(tmp_path / 'regridded_mesh')
    P.deltas_as_mesh(regridded, as_mesh, nlat, nlon)
    for r in ('0', '1'):
        clean.setenv('PGW_DELTA_RESIDENT', r)
        hp = P.run_files(ctx, p_paths, str(tmp_path / ('out_p' + r)), regridded)
        P.forget(s3)
        hm = P.run_files(ctx, m_paths, str(tmp_path / ('out_m' + r)), as_mesh)
        P.forget(s3)
        assert hp == hm and all(n >= 1 for n, _ in hp), 'n_iter / max_err histories'
        assert len(P.same_data(str(tmp_path / ('out_p' + r)), str(tmp_path / ('out_m' + r)))) == len(p_paths)


# ------------------------------------------------------------------ the command line on the 7 x 9 file
def _cli_pair(clean, tmp_path, extra=(), era_dtype=np.float64, name='rotated 7x9', zg_levels=None, span=None):
    """The command line on the point-wise files (deltas on their layout) and on mesh files that hold the same columns: the
    same return values, and output directories with the same files whose variables hold the same bytes."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    instants = P.INSTANTS[:2] if span is None else span
    outs = []
    for leg, layout in (('points', None), ('mesh', 'mesh')):
        era_dir, _, deltas = P.write_files(tmp_path, name, era_dtype, leg, layout=layout, instants=instants)
        if zg_levels is not None:
            P.keep_zg_levels(deltas, zg_levels)
        if 'interpolate_time' in extra:                                 # that mode also reads ps_delta.nc: a `ps` field on the layout
            shutil.copy(os.path.join(deltas, 'ps_historical.nc'), os.path.join(deltas, 'ps_delta.nc'))
        out = str(tmp_path / leg / 'out')
        args = ['-i', era_dir, '-H', '1', '-t', '-o', out, '-d', deltas] + list(extra)
        n = []
        if span is None:
            for t in instants:
                stamp = '{:%Y%m%d%H}'.format(t)
                n += list(s3._cli(args + ['-f', stamp, '-l', stamp]) or [])
        else:
            n = list(s3._cli(args + ['-f', '{:%Y%m%d%H}'.format(span[0]), '-l', '{:%Y%m%d%H}'.format(span[-1])]) or [])
        outs.append((out, n))
        P.forget(s3)
    assert outs[0][1] == outs[1][1]
    return P.same_data(outs[0][0], outs[1][0]), outs[0][1]


def test_cli_points_two_ranks(clean, tmp_path):
    """`-p 2`: the ranks the command line starts take the file's layout as the one-rank run does."""
    import datetime as dt
    from pgw4era5_amd import step_03_apply_to_era as s3
    span = (P.INSTANTS[0], P.INSTANTS[0] + dt.timedelta(hours=1))
    names, n = _cli_pair(clean, tmp_path, extra=['-p', '2'], span=span)
    assert len(names) == 2 and len(n) == 2 and all(k >= 1 for k in n)
    assert s3._DELTASETS == {}                                          # the ranks did the work


@pytest.mark.parametrize('debug', ['interpolate_full', 'interpolate_time'])
def test_cli_points_debug_mode(clean, tmp_path, debug):
    names, _ = _cli_pair(clean, tmp_path, extra=['-D', debug])
    assert len(names) == 2 * (7 if debug == 'interpolate_full' else 9)


def test_cli_points_local_p_ref_zg_on_its_own_axis(clean, tmp_path):
    """settings.p_ref_inp = None: the reference level is chosen per column among zg's levels, an axis of its own."""
    from pgw4era5_amd import settings as S
    clean.setattr(S, 'p_ref_inp', None)
    assert len(_cli_pair(clean, tmp_path, zg_levels=[0, 2, 3])[0]) == 2


def test_cli_points_reinterp(clean, tmp_path):
    from pgw4era5_amd import settings as S
    clean.setattr(S, 'i_reinterp', 1)
    assert len(_cli_pair(clean, tmp_path, era_dtype=np.float32)[0]) == 2


def test_cli_cells_f32_out_dtype(clean, tmp_path):
    """settings.f32_out_dtype = 'float32' on the cell list: the narrowed fields are written in the file's own shape."""
    from pgw4era5_amd import ncio, settings as S
    clean.setattr(S, 'f32_out_dtype', 'float32')
    names, _ = _cli_pair(clean, tmp_path, era_dtype=np.float32, name='cells 65')
    ds = ncio.open_dataset(os.path.join(str(tmp_path / 'points' / 'out'), names[0]), decode_times=False)
    assert ds['T'].dims == ('time', 'level', 'cell') and ds['T'].dtype.itemsize == 4 and ds['T'].shape == (1, P.NLEV, 65)


@pytest.mark.parametrize('name', ['rotated 7x9', 'cells 65'])
@pytest.mark.parametrize('storage', ['float64', 'float32', 'float32 narrowed'])
def test_point_files_through_the_raw_io_path(ctx, clean, tmp_path, name, storage):
    """With the fields counting as large (pinned buffers, big-endian bytes to and from the device, the one-row view of a
    cell list taken of those buffers) the output files are those of the host path, byte for byte, and every pinned buffer
    comes back to its pool."""
    from pgw4era5_amd import ncio, settings as S, step_03_apply_to_era as s3
    clean.setattr(S, 'f32_out_dtype', 'float32' if storage.endswith('narrowed') else 'float64')
    _, paths, deltas = P.write_files(tmp_path, name, np.dtype(storage.split()[0]), 'points', instants=P.INSTANTS[:2])
    clean.setenv('PGW_IO_RAW', '0')
    host = P.run_files(ctx, paths, str(tmp_path / 'host'), deltas, P.INSTANTS[:2])
    clean.setenv('PGW_IO_RAW', '1')
    clean.setattr(ncio, 'BIG_VARIABLE', 1024)
    raw = P.run_files(ctx, paths, str(tmp_path / 'raw'), deltas, P.INSTANTS[:2])
    pool = s3._pinned_pool(ctx)
    assert pool.allocated > 0 and sum(len(v) for v in pool._free.values()) == len(pool._owned)
    assert raw == host
    assert len(P.same_files(str(tmp_path / 'raw'), str(tmp_path / 'host'))) == 2


# ------------------------------------------------------------------ check_geopot
@pytest.mark.parametrize('name', ['rotated 7x9', 'cells 65'])
def test_check_geopot_on_a_point_file(ctx, clean, tmp_path, name):
    """The table and the zgcheck_ fields of the point-wise file pair equal those of the mesh run on the same columns."""
    from pgw4era5_amd import check_geopot as cg, ncio, step_03_apply_to_era as s3
    t = P.INSTANTS[0]
    res = {}
    for leg, layout in (('points', None), ('mesh', 'mesh')):
        _, paths, deltas = P.write_files(tmp_path, name, np.float64, leg, layout=layout, instants=(t,))
        out = str(tmp_path / leg / 'out')
        P.run_files(ctx, paths, out, deltas, (t,))
        chk = cg.check_path(str(tmp_path / leg), paths[0])
        table = cg.check_file(paths[0], os.path.join(out, os.path.basename(paths[0])), deltas, t, chk)
        P.forget(s3)
        res[leg] = (table, ncio.open_dataset(chk, decode_times=False))
    (tp, dp), (tm, dm) = res['points'], res['mesh']
    assert sorted(tp) == sorted(tm)
    for k in tp:
        a, b = (np.ascontiguousarray(x[k], dtype=np.float64) for x in (tp, tm))
        assert a.tobytes() == b.tobytes(), k
    assert int(np.asarray(tp['n_valid']).sum()) > 0
    hdims = ('rlat', 'rlon') if name.startswith('rotated') else ('cell',)
    for k in ('phi_change', 'phi_delta', 'phi_error'):
        assert dp[k].dims == ('time', 'plev') + hdims and dm[k].dims == ('time', 'plev', 'lat', 'lon')
        assert np.ascontiguousarray(dp[k].values).tobytes() == np.ascontiguousarray(dm[k].values).tobytes(), k


# ------------------------------------------------------------------ errors
def test_errors_before_any_launch(ctx, clean, tmp_path):
    """--bands on a point-wise file, lat over (rlat, rlon) beside lon over (rlon, rlat), a field that lacks a horizontal
    dimension: ValueError, nothing timed under any kernel, no output file."""
    from pgw4era5_amd import _lib, ncio, step_03_apply_to_era as s3
    era_dir, paths, deltas = P.write_files(tmp_path, 'rotated 7x9', np.float64, 'points', instants=P.INSTANTS[:1])
    out = tmp_path / 'out'
    span = ['-f', '2006072006', '-l', '2006072006', '-t']

    def variant(sub, edit):
        ds = ncio.open_dataset(paths[0], decode_times=False)
        edit(ds)
        d = str(tmp_path / sub)
        os.makedirs(d)
        ncio.to_netcdf(ds, os.path.join(d, os.path.basename(paths[0])))
        return d

    def cross(ds):
        ds['lon'] = ncio.Field(np.ascontiguousarray(ds['lon'].values.T), ('rlon', 'rlat'), {}, ds['lon'].attrs)

    def shorten(ds):
        ds['FIS'] = ncio.Field(ds['FIS'].values[:, 0, :], ('time', 'rlon'), {}, ds['FIS'].attrs)

    crossed, short = variant('crossed', cross), variant('short', shorten)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        with pytest.raises(ValueError, match='--bands on a point-wise file is not built'):
            s3._cli(['-i', era_dir, '-o', str(out), '-d', deltas, '--bands'] + span)
        for extra in ([], ['-D', 'interpolate_full']):
            with pytest.raises(ValueError, match='neither two 1-D axes of a mesh nor point-wise coordinates'):
                s3._cli(['-i', crossed, '-o', str(out), '-d', deltas] + span + extra)
            with pytest.raises(ValueError, match='FIS lies over'):
                s3._cli(['-i', short, '-o', str(out), '-d', deltas] + span + extra)
        assert [k for k in _lib.KERNEL_IDS if ctx.profile_get(k)[0] != 0] == []
    finally:
        ctx.profile(False)
    assert not out.exists() or os.listdir(str(out)) == []
    assert s3._DELTASETS == {}
