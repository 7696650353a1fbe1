"""The rotation of wind components onto a rotated-pole grid, stated in numpy, and the files the step_02 tests run on.
tests/test_wind_rotation_host.py ties the statement to the grid's own geometry; tests/test_wind_rotation_hip.py holds the
kernels (k_wind_rotation, k_rotate_pair, k_regrid_points_wind) to it.  No GPU is needed in this file.

`rotation` is the definition - degrees in, radians inside; the target at geographic (lat, lon), the north pole of the rotated
grid at geographic (pole_lat, pole_lon) (COSMO's uv2uvrot):
    D  = pole_lon - lon
    a1 = cos(pole_lat) sin(D)
    a2 = sin(pole_lat) cos(lat) - cos(pole_lat) sin(lat) cos(D)
    rho = sqrt(a1^2 + a2^2)               (the cosine of the point's rotated latitude)
    c = a2 / rho,  s = a1 / rho           rho == 0: (1, 0);  a NaN coordinate: NaN
`rotate` applies it: u_rot = u c - v s, v_rot = u s + v c in float64, rounded once to the storage type; the inverse is
u = u_rot c + v_rot s, v = -u_rot s + v_rot c."""
import os

import numpy as np

from pgw4era5_amd import ncio, settings, synthetic

POLES = [(39.25, -162.0), (43.0, -170.0), (-30.0, 20.0), (6.55, 0.0), (90.0, -180.0)]
NPOINTS = [1, 63, 64, 65, 257, 513]


# ------------------------------------------------------------------ the statement
def rotation(lat, lon, pole_lat, pole_lon):
    """-> (c, s, rho), float64 arrays of the coordinates' shape."""
    phi, phip = np.deg2rad(np.asarray(lat, dtype=np.float64)), np.deg2rad(float(pole_lat))
    d = np.deg2rad(float(pole_lon) - np.asarray(lon, dtype=np.float64))
    a1 = np.cos(phip) * np.sin(d)
    a2 = np.sin(phip) * np.cos(phi) - np.cos(phip) * np.sin(phi) * np.cos(d)
    rho = np.sqrt(a1 * a1 + a2 * a2)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.where(rho == 0.0, 1.0, a2 / np.where(rho == 0.0, 1.0, rho))
        s = np.where(rho == 0.0, 0.0, a1 / np.where(rho == 0.0, 1.0, rho))
    return c, s, rho


def rotate(u, v, c, s, inverse=False):
    """u, v (..., S) with c, s of shape S -> (u', v') in the common dtype of u and v (float32 only when both are)."""
    u, v = np.asarray(u), np.asarray(v)
    dtype = np.float32 if u.dtype == v.dtype == np.float32 else np.float64
    u, v = u.astype(np.float64), v.astype(np.float64)
    with np.errstate(invalid='ignore'):
        if inverse:
            return (u * c + v * s).astype(dtype), (-u * s + v * c).astype(dtype)
        return (u * c - v * s).astype(dtype), (u * s + v * c).astype(dtype)


def grid_east(nrlat, nrlon, pole, h=1e-4):
    """Unit vector (east, north) of increasing rlon in the geographic tangent plane at the points of
    synthetic.rotated_pole_grid(nrlat, nrlon, pole), by central differences of the grid's own lat / lon."""
    r0, r1 = -22.0, 22.0
    _, _, la_m, lo_m = synthetic.rotated_pole_grid(nrlat, nrlon, *pole, rlon_range=(r0 - h, r1 - h))
    _, _, la_p, lo_p = synthetic.rotated_pole_grid(nrlat, nrlon, *pole, rlon_range=(r0 + h, r1 + h))
    _, _, lat, _ = synthetic.rotated_pole_grid(nrlat, nrlon, *pole, rlon_range=(r0, r1))
    dlon = (lo_p - lo_m + 180.0) % 360.0 - 180.0                        # across +-180
    e, n = np.cos(np.deg2rad(lat)) * dlon, la_p - la_m
    norm = np.hypot(e, n)
    return e / norm, n / norm


def points(n, pole, seed=0):
    """n points of a rotated grid with north pole `pole`, |rlat| <= 14 (rho = cos(rlat) >= 0.97), in random order:
    (lat, lon, rlat)."""
    rng = np.random.default_rng(seed + n)
    rlat, rlon = rng.uniform(-14.0, 14.0, n), rng.uniform(-22.0, 22.0, n)
    lat, lon = np.empty(n), np.empty(n)
    for k in range(n):                                                   # one point per call: rotated_pole_grid makes meshes
        _, _, la, lo = synthetic.rotated_pole_grid(1, 1, *pole, rlat_range=(rlat[k], rlat[k]), rlon_range=(rlon[k], rlon[k]))
        lat[k], lon[k] = la[0, 0], lo[0, 0]
    return lat, lon, rlat


def same_bits(a, b):
    """dtype, shape, NaN mask and the bits of every other value equal (which NaN comes out of a NaN is left open)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg='NaN mask')
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    ok = ~np.isnan(a)
    np.testing.assert_array_equal(a.view(u)[ok], b.view(u)[ok])


# ------------------------------------------------------------------ files of the step_02 tests
POLE = (39.25, -162.0)                       # of synthetic.rotated_pole_grid and of the files write_case_files(layout='rotated') writes
PLEV = np.array([85000.0, 50000.0])
TIMES = np.array(['1995-%02d-15T12:00:00' % (m + 1) for m in range(3)], dtype='datetime64[s]')


def source_axes(nlat=13, nlon=24):
    """A regular regional grid around the 7 x 9 rotated target."""
    return np.linspace(20.0, 75.0, nlat), np.linspace(-50.0, 70.0, nlon)


def write_sources(gcm, variables=('ua', 'va', 'ta'), dtype=np.float32, nlat=13, nlon=24, edit=None):
    """{var}_delta.nc and {var}_historical.nc for ua / va - the solid-body rotation about POLE, scaled per record and level -
    and ta.  edit(var, ds): last changes to a dataset before it is written."""
    os.makedirs(gcm, exist_ok=True)
    lat, lon = source_axes(nlat, nlon)
    u, v = synthetic.solid_body_wind(lat[:, None], lon[None, :], *POLE)
    scale = (1.0 + 0.25 * np.arange(len(TIMES)))[:, None, None, None] * np.array([3.0, 11.0])[None, :, None, None]
    fields = dict(ua=scale * u[None, None], va=scale * v[None, None], ta=scale * (1.0 + 0.01 * lat[:, None] + 0.02 * lon[None, :]))
    for k, base in enumerate(settings.file_name_bases.values()):
        for var in variables:
            ds = ncio.Dataset(attrs=dict(title='winds of a solid-body rotation'))
            ds['time'] = ncio.Field(TIMES, ('time',))
            ds['plev'] = ncio.Field(PLEV, ('plev',), attrs=dict(units='Pa'))
            ds['lat'] = ncio.Field(lat, ('lat',), attrs=dict(units='degrees_north'))
            ds['lon'] = ncio.Field(lon, ('lon',), attrs=dict(units='degrees_east'))
            ds[var] = ncio.Field(((1 + k) * fields[var]).astype(dtype), ('time', 'plev', 'lat', 'lon'),
                                 {'time': TIMES, 'plev': PLEV}, dict(units='m s-1' if var != 'ta' else 'K'))
            if edit is not None:
                edit(var, ds)
            ncio.to_netcdf(ds, os.path.join(gcm, base.format(var)))
    return lat, lon


def write_target(tmp, layout='rotated'):
    """The ERA5-like target file of synthetic.write_case_files on a 7 x 9 grid -> path."""
    case = synthetic.make_case(nlat=7, nlon=9, nlev=6, seed=3, dtype=np.float32, plev=PLEV)
    return synthetic.write_case_files(case, os.path.join(tmp, 'era_' + layout), os.path.join(tmp, 'unused_deltas_' + layout), layout=layout)


def write_bare_target(path, mappings, u_names=None):
    """A 7 x 9 rotated target with 2-D lat / lon, a variable U and one scalar mapping variable per entry of `mappings`
    ({name: attributes}); U names `u_names` as its grid_mapping when given."""
    rlat, rlon, lat, lon = synthetic.rotated_pole_grid(7, 9)
    ds = ncio.Dataset()
    ds['rlat'] = ncio.Field(rlat, ('rlat',))
    ds['rlon'] = ncio.Field(rlon, ('rlon',))
    ds['lat'] = ncio.Field(lat, ('rlat', 'rlon'))
    ds['lon'] = ncio.Field(lon, ('rlat', 'rlon'))
    for name, attrs in mappings.items():
        ds[name] = ncio.Field(np.array(b'', dtype='S1'), (), attrs=attrs)
    ds['U'] = ncio.Field(np.zeros((7, 9), np.float32), ('rlat', 'rlon'), attrs=dict(grid_mapping=u_names) if u_names else {})
    ncio.to_netcdf(ds, path)
    return path
