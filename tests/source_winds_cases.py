"""Winds of a rotated-pole SOURCE grid through the curvilinear regridding (`step_02 regridding --source_winds` with
settings.i_use_xesmf_regridding = 1): the numpy statement of the definition, targets, and the files the step_02 tests run on.
tests/test_source_winds_host.py ties the statement to a flow with a known answer; tests/test_source_winds_hip.py holds
k_row_mean_plain_wind / k_regrid_sparse_wind to the composed form through the existing entries.  No GPU is needed in this file.

The definition (include/pgw_hip.h above pgw_regrid_sparse_wind), T the common dtype of ua and va:
    ug, vg = rotate(ua, va, cs_s, sn_s, inverse=True)            left out when the source winds are geographic
    ur, vr = apply(ug), apply(vg)                                the weights of the curvilinear locate phase
    u,  v  = rotate(ur, vr, cs_t, sn_t)                          left out when the outputs stay geographic
each line rounded to T."""
import os

import numpy as np

import test_regrid_curvilinear_host as H
import wind_rotation_cases as W
from pgw4era5_amd import ncio, settings, synthetic

SOURCE_POLE = (39.25, -162.0)                # of synthetic.rotated_pole_grid's default grid and of make_rotated_delta's files
TARGET_POLE = (43.0, -170.0)                 # of the rotated target of the step_02 tests


def statement(ua, va, idx, w, src=None, targ=None, unmapped_nan=False):
    """ua, va (nfield, ny, nx); src = (cos, sin) over (ny, nx) or None; targ = (cos, sin) over (nt,) or None -> (u, v)
    (nfield, nt) in the common dtype, from W.rotate and H.apply_statement."""
    ua, va = np.asarray(ua), np.asarray(va)
    dtype = np.float32 if ua.dtype == va.dtype == np.float32 else np.float64
    u, v = W.rotate(ua, va, src[0], src[1], inverse=True) if src is not None else (ua.astype(dtype), va.astype(dtype))
    u, v = H.apply_statement(u, idx, w, unmapped_nan), H.apply_statement(v, idx, w, unmapped_nan)
    return W.rotate(u, v, targ[0], targ[1]) if targ is not None else (u, v)


def angles(shape, seed):
    """(cos, sin) of arbitrary angles of the given shape: any unit pair is a valid rotation for a comparison of bits."""
    th = np.random.default_rng(seed).uniform(-np.pi, np.pi, shape)
    return np.cos(th), np.sin(th)


def targets(X, periodic, nt, seed):
    """nt targets: known cells (cap triangles of a periodic grid among them), source nodes, points anywhere on the sphere
    (unmapped ones on a regional grid) - repeated up to nt."""
    P, _, _ = H.truth_targets(X, periodic, min(nt, 65), seed)
    nodes = X.reshape(-1, 3)[::max(1, X.shape[0] * X.shape[1] // 16)]
    anywhere = H.normalise(np.random.default_rng(seed).standard_normal((16, 3)))
    P = np.concatenate([P, nodes, anywhere], axis=0)
    return np.concatenate([P] * (nt // len(P) + 1), axis=0)[:nt]


def solid_body_case(nt=257, seed=12):
    """The solid-body flow about the pole of the rot24x48 grid: grid-relative (cos rlat, 0) on that grid, its analytic
    geographic components at the nodes, the source rotation, and nt targets inside the grid.
    -> dict(X, P, lat, lon, grid (u, v), geo (u, v), src (cos, sin))."""
    rlat, _, lat, lon = synthetic.rotated_pole_grid(24, 48)
    X, periodic = H.GRIDS['rot24x48']()
    P, _, _ = H.truth_targets(X, periodic, nt, seed)
    c, s, _ = W.rotation(lat, lon, *SOURCE_POLE)
    grid = (np.broadcast_to(np.cos(np.deg2rad(rlat))[:, None], lat.shape).copy()[None], np.zeros(lat.shape)[None])
    geo = tuple(x[None] for x in synthetic.solid_body_wind(lat, lon, *SOURCE_POLE))
    return dict(X=X, P=P, lat=lat, lon=lon, grid=grid, geo=geo, src=(c, s))


# ------------------------------------------------------------------ files of the step_02 tests
def with_mapping(ds, var_name, pole=SOURCE_POLE):
    """The dataset with a scalar `rotated_pole` mapping variable and `grid_mapping` on `var_name`, as CORDEX files carry them."""
    ds['rotated_pole'] = ncio.Field(np.array(b'', dtype='S1'), (), attrs=dict(
        grid_mapping_name='rotated_latitude_longitude', grid_north_pole_latitude=np.float64(pole[0]),
        grid_north_pole_longitude=np.float64(pole[1])))
    f = ds[var_name]
    ds[var_name] = ncio.Field(f.values, f.dims, f.coords, dict(f.attrs, grid_mapping='rotated_pole'), var_name)
    return ds


def write_sources(gcm, variables=('ua', 'va', 'ta'), dtype=np.float32, mapping=True, edit=None, **shape):
    """{var}_delta.nc and {var}_historical.nc of synthetic.make_rotated_delta on its default rotated grid (pole SOURCE_POLE),
    ua / va with the rotated mapping.  edit(var, ds): last changes before a dataset is written."""
    os.makedirs(gcm, exist_ok=True)
    for k, base in enumerate(settings.file_name_bases.values()):
        for j, var in enumerate(variables):
            ds = synthetic.make_rotated_delta(dtype=dtype, var_name=var, seed=10 * k + j, **shape)
            if mapping and var != 'ta':
                with_mapping(ds, var)
            if edit is not None:
                edit(var, ds)
            ncio.to_netcdf(ds, os.path.join(gcm, base.format(var)))
    return gcm


def write_mesh_target(path):
    """A small lat-lon mesh inside the source domain."""
    ds = ncio.Dataset()
    lat, lon = np.linspace(44.0, 57.0, 8), np.linspace(6.0, 30.0, 11)
    ds['lat'] = ncio.Field(lat, ('lat',), {'lat': lat}, dict(units='degrees_north'))
    ds['lon'] = ncio.Field(lon, ('lon',), {'lon': lon}, dict(units='degrees_east'))
    ncio.to_netcdf(ds, path)
    return path


def write_rotated_target(path, pole=TARGET_POLE, mapping=True):
    """A 7 x 9 rotated target with another pole inside the source domain: 2-D lat / lon, a variable U, the rotated mapping."""
    rlat, rlon, lat, lon = synthetic.rotated_pole_grid(7, 9, *pole, rlat_range=(-4.0, 4.0), rlon_range=(-3.0, 9.0))
    ds = ncio.Dataset()
    ds['rlat'] = ncio.Field(rlat, ('rlat',))
    ds['rlon'] = ncio.Field(rlon, ('rlon',))
    ds['lat'] = ncio.Field(lat, ('rlat', 'rlon'))
    ds['lon'] = ncio.Field(lon, ('rlat', 'rlon'))
    ds['U'] = ncio.Field(np.zeros((7, 9), np.float32), ('rlat', 'rlon'))
    if mapping:
        with_mapping(ds, 'U', pole)
    ncio.to_netcdf(ds, path)
    return path
