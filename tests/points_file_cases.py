"""Cases and helpers of tests/test_step03_points_hip.py and tests/test_step03_points_host.py: step_03 on ERA5 files whose
lat / lon are 2-D over shared dimensions (a rotated-pole file) or 1-D over one `cell` dimension.

Everything here is host code.  The reference of every comparison is step_03 on a MESH file that holds the same columns and
the same deltas - the code path that was there before.  All comparisons are for equal bytes, so no tolerance is derived.
`conditions()` asserts on the CPU what the cases exist for."""
import os

import numpy as np

import source_delta_cases as K

BLOCK = 256                                  # threads per block of the column kernels

# ------------------------------------------------------------------ file cases
PLEV5 = np.array([100000.0, 70000.0, 30000.0, 10000.0, 1000.0])            # settings.p_ref_inp = 30000 is one of them
NLEV = 12
INSTANTS = K.INSTANTS
FILES = {'rotated 7x9': ('rotated', 7, 9), 'rotated 11x24': ('rotated', 11, 24), 'cells 65': ('cells', 5, 13)}
PERM = np.random.default_rng(65).permutation(65)                             # the cell list's order of the 5 x 13 mesh's columns


def _permuted_row(a, nlat, nlon):
    a = np.asarray(a)
    if a.ndim >= 3 and a.shape[-2:] == (nlat, nlon):
        return np.ascontiguousarray(a.reshape(a.shape[:-2] + (1, nlat * nlon))[..., PERM])
    return a


def file_case(name, instant, dtype, seed=11):
    """A synthetic ERA5 case (12 levels, deltas on 5 levels) for the file `name`.  Rotated files: nlat x nlon columns whose 2-D
    lat / lon are synthetic.rotated_pole_grid's.  The cell list: the columns of a 5 x 13 mesh over Europe in the order PERM, as
    a case of ONE row - `lat2d` / `lon2d` are the (1, 65) coordinates of the cells."""
    from pgw4era5_amd import synthetic
    layout, nlat, nlon = FILES[name]
    c = synthetic.make_case(nlat, nlon, NLEV, seed=seed, dtype=dtype, plev=PLEV5, target_dt=instant)
    if layout == 'cells':
        lat, lon = np.linspace(35.0, 62.0, nlat), np.linspace(-12.0, 31.0, nlon)
        la, lo = np.meshgrid(lat, lon, indexing='ij')
        c['era'] = {k: _permuted_row(v, nlat, nlon) for k, v in c['era'].items()}
        c['deltas'] = {k: _permuted_row(v, nlat, nlon) for k, v in c['deltas'].items()}
        c['lat2d'], c['lon2d'] = la.reshape(1, -1)[:, PERM], lo.reshape(1, -1)[:, PERM]
        c['lat'], c['lon'] = np.array([0.0]), np.arange(nlat * nlon) * 1.0             # the stand-in axes of the one-row mesh
    return c, layout


def conditions():
    """What the cases above exist for, asserted as counts on the CPU."""
    # the files: 63 columns (below a wave), 264 columns (two blocks, the last ragged), 65 cells in an order of their own
    cols = {k: v[1] * v[2] for k, v in FILES.items()}
    assert cols == {'rotated 7x9': 63, 'rotated 11x24': 264, 'cells 65': 65}
    assert cols['rotated 11x24'] > BLOCK and cols['rotated 11x24'] % BLOCK != 0
    assert sorted(PERM.tolist()) == list(range(65)) and not np.array_equal(PERM, np.arange(65))
    assert len(PLEV5) == 5 and 30000.0 in PLEV5
    return cols


# ------------------------------------------------------------------ helpers of the GPU tests
def forget(s3):
    for d in s3._DELTASETS.values():
        d.free()
    s3._DELTASETS.clear()


def run_files(ctx, paths, out_dir, delta_dir, instants=INSTANTS):
    """pgw_for_era5 file by file -> [(n_iter, max_err history)]."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    os.makedirs(out_dir, exist_ok=True)
    hist = []
    for p, t in zip(paths, instants):
        n = s3.pgw_for_era5(p, os.path.join(out_dir, os.path.basename(p)), delta_dir, t, True)
        a = ctx._last_file_args
        assert n == a.n_iter
        hist.append((int(a.n_iter), [float(x) for x in a.max_err_hist[:min(a.n_iter, 32)]]))
    return hist


def same_files(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b))
    for n in names:
        assert open(os.path.join(a, n), 'rb').read() == open(os.path.join(b, n), 'rb').read(), n
    return names


def variables(path):
    """name -> (dims, dtype, data bytes, attribute names) of every variable of a file, as stored."""
    from pgw4era5_amd import ncio
    ds = ncio.open_dataset(path, decode_times=False, decode_mask_scale=False)
    return {k: (v.dims, v.values.dtype.str, np.ascontiguousarray(v.values).tobytes(), sorted(v.attrs)) for k, v in ds.variables.items()}


def same_data(a, b, skip=('lat', 'lon')):
    """The two directories hold files of the same names whose common variables (but the coordinates) have the same dtype and
    data bytes; at least one of them per file lies over horizontal dimensions."""
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b))
    for n in names:
        va, vb = variables(os.path.join(a, n)), variables(os.path.join(b, n))
        common = [k for k in va if k in vb and k not in skip]
        assert any(len(va[k][0]) >= 2 for k in common), n
        for k in common:
            assert va[k][1:3] == vb[k][1:3], (n, k)
    return names


def write_files(tmp_path, name, dtype, leg, layout=None, instants=INSTANTS):
    """The ERA5 files of the case `name` (and the deltas on their layout) under tmp_path/leg -> (era dir, paths, delta dir)."""
    from pgw4era5_amd import synthetic
    era, deltas = str(tmp_path / leg / 'era'), str(tmp_path / leg / 'deltas')
    paths = []
    for t in instants:
        case, point_layout = file_case(name, t, dtype)
        paths.append(synthetic.write_case_files(case, era, deltas, layout=point_layout if layout is None else layout))
    return era, paths, deltas


def gcm_files(tmp_path, **rewrite):
    """The input of `step_02 regridding` on a 12 x 24 source with the five delta levels."""
    from pgw4era5_amd import synthetic
    d = str(tmp_path / 'gcm')
    synthetic.write_gcm_files(d, nlat=12, nlon=24, plev=PLEV5, seed=5, ocean=(12, 16))
    if rewrite:
        K.rewrite(d, **rewrite)
    return d


def regrid_onto(tmp_path, gcm, example):
    """`step_02 regridding -e example` with all default variables -> the directory it wrote."""
    from pgw4era5_amd import step_02_preproc_deltas as s2
    d = str(tmp_path / 'regridded')
    assert len(s2.main(['regridding', '-i', gcm, '-o', d, '-e', example])) == 22
    return d


def deltas_as_mesh(src, dst, nlat, nlon):
    """The delta files of `src` (on a point-wise layout) with the same arrays over (lat, lon) and stand-in axes."""
    from pgw4era5_amd import ncio
    os.makedirs(dst, exist_ok=True)
    for fname in sorted(os.listdir(src)):
        ds = ncio.open_dataset(os.path.join(src, fname), decode_times=False, decode_mask_scale=False)
        var = fname.split('_')[0]
        f = ds[var]
        lead = tuple(d for d in f.dims if d in ('time', 'plev'))
        assert f.dims[:len(lead)] == lead and int(np.prod(f.shape[len(lead):])) == nlat * nlon
        out = ncio.Dataset()
        for d in lead:
            out[d] = ds[d]
        out['lat'] = ncio.Field(np.linspace(-1.0, 1.0, nlat) if nlat > 1 else np.array([0.0]), ('lat',))
        out['lon'] = ncio.Field(np.arange(nlon) * 1.0, ('lon',))
        out[var] = ncio.Field(np.asarray(f.values).reshape(f.shape[:len(lead)] + (nlat, nlon)), lead + ('lat', 'lon'), {}, f.attrs)
        ncio.to_netcdf(out, os.path.join(dst, fname))


def keep_zg_levels(delta_dir, levels):
    """zg_delta.nc of the directory cut to these indices of its plev axis: an axis of its own."""
    from pgw4era5_amd import ncio
    path = os.path.join(delta_dir, 'zg_delta.nc')
    ds = ncio.open_dataset(path, decode_times=False, decode_mask_scale=False)
    f = ds['zg']
    ds['plev'] = ncio.Field(np.asarray(ds['plev'].values)[levels], ('plev',), attrs=ds['plev'].attrs)
    ds['zg'] = ncio.Field(np.ascontiguousarray(np.asarray(f.values)[:, levels]), f.dims, {}, f.attrs)
    ncio.to_netcdf(ds, path)
