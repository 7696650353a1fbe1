"""tos / siconc onto targets with 2-D coordinates on the GPU: `pgw_ocean_targets` and `pgw_gauss_interp_points` through the
C API, `functions.gauss_interp_points` / `nan_ignoring_interp`, and `step_02 regridding` onto an extpar file.

The points entry orders its targets by the cell of the source grid on the device and writes every result to the target's
own index; per target the accepted source points arrive in the same order whatever block the target ends up in, so the
yardstick at the kernel level is `pgw_gauss_interp` on the same (tx, ty) in the caller's order, BIT FOR BIT.  Against the
longdouble restatement (`gauss_reference`) the bound is `_check_gauss`'s derived one, (n_acc + 40) eps scale; against the
oracle the project's tolerance for this kernel, rtol 1e-10 (tests/test_ocean_interp.py).  Each case asserts its own
intended condition from its inputs."""
import numpy as np
import pytest

from test_step02_kernels_hip import BLOCK, SENTINEL, Cloud, _assert_same_bits, _background, _check_gauss, _gauss
from oracle import pgw_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    return default_context()


def _points(ctx, cloud, tx, ty, sv=None, radius=1.0, sharpness=4.0, nfield=None, cell=None, ntarg=None):
    """One pgw_gauss_interp_points call on a sentinel-filled buffer: out [nm, ntarg]."""
    sv = cloud.sv if sv is None else np.ascontiguousarray(sv, dtype=np.float64)
    nm = sv.shape[1] if nfield is None else nfield
    tx, ty = np.ascontiguousarray(tx, dtype=np.float64), np.ascontiguousarray(ty, dtype=np.float64)
    nsrc = len(cloud.sx)
    assert sv.shape[0] == nsrc and len(ty) == len(tx)
    d_tx, d_ty = ctx.to_device(tx), ctx.to_device(ty)
    d_cs = ctx.empty(cloud.cell_start.shape, np.int32).copy_from(cloud.cell_start)
    d_sx, d_sy = ctx.to_device(cloud.sx if nsrc else np.zeros(1)), ctx.to_device(cloud.sy if nsrc else np.zeros(1))
    d_sv = ctx.to_device(sv if nsrc else np.zeros((1, max(nm, 1))))
    d_out = ctx.to_device(np.full((max(nm, 1), len(tx)), SENTINEL))
    ctx._check(ctx.lib.pgw_gauss_interp_points(ctx.handle, len(tx) if ntarg is None else ntarg, d_tx.ptr, d_ty.ptr, cloud.ncx,
                                               cloud.ncy, cloud.x0, cloud.y0, cloud.h if cell is None else cell, d_cs.ptr, nsrc,
                                               d_sx.ptr, d_sy.ptr, d_sv.ptr, nm, float(radius), float(sharpness), d_out.ptr))
    return d_out.numpy()


def _same_as_mesh_entry(ctx, cloud, tx, ty, **kw):
    """The points entry against pgw_gauss_interp on the same targets, bit for bit; no sentinel left.  Returns the result."""
    got = _points(ctx, cloud, tx, ty, **kw)
    assert not (got == SENTINEL).any()
    _assert_same_bits(got, _gauss(ctx, cloud, tx, ty, **kw), 'points entry against pgw_gauss_interp')
    return got


@pytest.fixture(scope='module')
def cloud():
    return Cloud(*_background(np.random.default_rng(50), 10, 3, nan_fraction=0.05))


def _keys(cloud, tx, ty):
    cx, cy = cloud.target_cells(tx, ty)
    return np.clip(cx, -1, cloud.ncx), np.clip(cy, -1, cloud.ncy)


# ------------------------------------------------------------------ pgw_gauss_interp_points against pgw_gauss_interp
@pytest.mark.parametrize('ntarg', [1, 255, 256, 257, 600])
def test_points_block_boundaries(ctx, cloud, ntarg):
    rng = np.random.default_rng(ntarg)
    tx, ty = rng.uniform(-0.4, 6.4, ntarg), rng.uniform(-0.4, 6.4, ntarg)
    got = _same_as_mesh_entry(ctx, cloud, tx, ty)
    assert got.shape == (3, ntarg) and not np.isnan(got).all()
    assert -(-ntarg // BLOCK) == {1: 1, 255: 1, 256: 1, 257: 2, 600: 3}[ntarg]


def test_points_in_a_random_permutation(ctx, cloud):
    rng = np.random.default_rng(1)
    tx, ty = rng.uniform(0.0, 6.0, 600), rng.uniform(0.0, 6.0, 600)
    p = rng.permutation(600)
    assert (p != np.arange(600)).sum() > 590
    a, b = _same_as_mesh_entry(ctx, cloud, tx, ty), _same_as_mesh_entry(ctx, cloud, tx[p], ty[p])
    _assert_same_bits(b, np.ascontiguousarray(a[:, p]), 'a target keeps its bits wherever it stands')
    assert not np.isnan(a).any()


def test_points_alternating_between_two_far_cells(ctx, cloud):
    rng = np.random.default_rng(2)
    n = 300
    tx = np.where(np.arange(n) % 2 == 0, rng.uniform(0.0, 1.0, n), rng.uniform(5.0, 6.0, n))
    ty = np.where(np.arange(n) % 2 == 0, rng.uniform(0.0, 1.0, n), rng.uniform(5.0, 6.0, n))
    cx, cy = _keys(cloud, tx, ty)
    assert (cx[0::2] == 0).all() and (cy[0::2] == 0).all() and (cx[1::2] == 5).all() and (cy[1::2] == 5).all()
    got = _same_as_mesh_entry(ctx, cloud, tx, ty)
    assert not np.isnan(got).any()


def test_points_one_target_in_every_cell(ctx, cloud):
    rng = np.random.default_rng(3)
    gx, gy = np.meshgrid(np.arange(6), np.arange(6), indexing='ij')
    p = rng.permutation(36)
    tx, ty = (gx.ravel() + rng.uniform(0.0, 1.0, 36))[p], (gy.ravel() + rng.uniform(0.0, 1.0, 36))[p]
    cx, cy = _keys(cloud, tx, ty)
    assert len(set(zip(cx, cy))) == 36
    _same_as_mesh_entry(ctx, cloud, tx, ty)


def test_points_one_cell_fills_three_blocks(ctx, cloud):
    rng = np.random.default_rng(4)
    tx, ty = rng.uniform(2.0, 3.0, 600), rng.uniform(4.0, 5.0, 600)
    cx, cy = _keys(cloud, tx, ty)
    assert (cx == 2).all() and (cy == 4).all() and -(-600 // BLOCK) == 3
    got = _same_as_mesh_entry(ctx, cloud, tx, ty)
    assert not np.isnan(got).any()


def test_points_every_third_target_inactive(ctx, cloud):
    rng = np.random.default_rng(5)
    tx, ty = rng.uniform(0.0, 6.0, 600), rng.uniform(0.0, 6.0, 600)
    tx[0::6] = np.nan
    ty[3::6] = np.nan                                              # either coordinate
    inactive = np.isnan(tx) | np.isnan(ty)
    n_active = int((~inactive).sum())
    assert inactive[0::3].all() and n_active == 400 and n_active % BLOCK != 0
    got = _same_as_mesh_entry(ctx, cloud, tx, ty)
    assert np.isnan(got[:, inactive]).all() and not np.isnan(got[:, ~inactive]).any()


@pytest.mark.parametrize('ntarg', [5, 300])
def test_points_all_inactive(ctx, cloud, ntarg):
    got = _points(ctx, cloud, np.full(ntarg, np.nan), np.full(ntarg, np.nan))
    assert got.shape == (3, ntarg) and np.isnan(got).all()


def test_points_outside_the_cell_grid(ctx, cloud):
    """On each of the four sides: within one radius of the border cells' points, one cell further out, and at +-1e18."""
    rng = np.random.default_rng(6)
    n = 40
    along = rng.uniform(0.5, 5.5, n)
    near = [(np.full(n, -0.05), along), (np.full(n, 6.05), along), (along, np.full(n, -0.05)), (along, np.full(n, 6.05))]
    far = [(np.full(n, -1.5), along), (np.full(n, 7.5), along), (along, np.full(n, -1.5)), (along, np.full(n, 7.5))]
    tx = np.concatenate([a for a, _ in near + far] + [rng.uniform(0.0, 6.0, 60)])
    ty = np.concatenate([b for _, b in near + far] + [rng.uniform(0.0, 6.0, 60)])
    p = rng.permutation(len(tx))
    tx, ty = tx[p], ty[p]
    cx, cy = cloud.target_cells(tx, ty)
    outside = (cx < 0) | (cx >= 6) | (cy < 0) | (cy >= 6)
    ring = outside & (cx >= -1) & (cx <= 6) & (cy >= -1) & (cy <= 6)
    assert ring.sum() == 4 * n and (outside & ~ring).sum() == 4 * n
    for side in ((cx == -1), (cx == 6), (cy == -1), (cy == 6), (cx == -2), (cx == 7), (cy == -2), (cy == 7)):
        assert side.sum() == n
    got = _same_as_mesh_entry(ctx, cloud, tx, ty)
    _, n_acc, _ = _check_gauss(got, cloud, tx, ty)
    assert (n_acc[:, ring].max(axis=0) > 0).all()                  # found by the border cells' points
    assert (n_acc[:, outside & ~ring] == 0).all() and np.isnan(got[:, outside & ~ring]).all()
    # far away: the same targets plus one at +-1e18 on each side and in the corners; no error status, NaN there, the others keep their bits
    big = 1e18
    fx = np.array([-big, big, 3.0, 3.0, -big, big, big, -big])
    fy = np.array([3.0, 3.0, -big, big, -big, big, -big, big])
    pos = np.sort(rng.choice(len(tx), len(fx), replace=False))
    tx2, ty2 = np.insert(tx, pos, fx), np.insert(ty, pos, fy)
    is_far = np.abs(tx2) + np.abs(ty2) >= big
    assert is_far.sum() == len(fx) and np.isfinite(tx2).all() and np.isfinite(ty2).all()
    got2 = _points(ctx, cloud, tx2, ty2)
    assert np.isnan(got2[:, is_far]).all() and not (got2 == SENTINEL).any()
    _assert_same_bits(np.ascontiguousarray(got2[:, ~is_far]), got, 'targets sharing a call with far-away ones')


# ------------------------------------------------------------------ against the longdouble reference
def test_points_nan_months_and_a_coincident_target(ctx):
    rng = np.random.default_rng(7)
    bx, by, bv = _background(rng, 6, 3, nan_fraction=0.1)
    cloud = Cloud(np.concatenate([bx, [2.5]]), np.concatenate([by, [3.25]]), np.concatenate([bv, [[1.5, np.nan, -2.5]]]))
    tx, ty = rng.uniform(-0.5, 6.5, 300), rng.uniform(-0.5, 6.5, 300)
    tx[200], ty[200] = 2.5, 3.25
    assert np.isnan(cloud.sv).any(axis=1).sum() > 20
    got = _points(ctx, cloud, tx, ty)
    _, n_acc, hits = _check_gauss(got, cloud, tx, ty)
    assert hits[:, 200].tolist() == [True, False, True] and hits.sum() == 2
    _assert_same_bits(got[[0, 2], 200], np.array([1.5, -2.5]))
    assert not np.isnan(got[1, 200]) and n_acc[1, 200] >= 3          # month 1 of that point is NaN: a weighted mean of the others
    assert (n_acc[0] != n_acc[1]).any()                            # months with their own NaN points


@pytest.mark.parametrize('nm', [1, 16])
def test_points_number_of_fields(ctx, nm):
    rng = np.random.default_rng(20 + nm)
    cloud = Cloud(*_background(rng, 8, nm, nan_fraction=0.05))
    tx, ty = rng.uniform(-1.2, 7.2, 300), rng.uniform(-1.2, 7.2, 300)
    got = _points(ctx, cloud, tx, ty)
    assert got.shape == (nm, 300)
    _, n_acc, _ = _check_gauss(got, cloud, tx, ty)
    assert (n_acc.max(axis=0) == 0).sum() >= 3 and (n_acc.min(axis=0) > 0).sum() >= 200


# ------------------------------------------------------------------ workspace, repeatability, argument errors
def test_points_workspace_grows_and_is_reused(ctx, cloud):
    rng = np.random.default_rng(8)
    for ntarg in (2000, 10, 3000):
        tx, ty = rng.uniform(-0.5, 6.5, ntarg), rng.uniform(-0.5, 6.5, ntarg)
        tx[::7] = np.nan
        got = _same_as_mesh_entry(ctx, cloud, tx, ty)
        _assert_same_bits(_points(ctx, cloud, tx, ty), got, 'the same call twice')
        if ntarg == 10:
            _check_gauss(got, cloud, tx, ty)


def test_points_argument_errors(ctx, cloud):
    rng = np.random.default_rng(9)
    tx, ty = rng.uniform(0.0, 6.0, 50), rng.uniform(0.0, 6.0, 50)
    good = _same_as_mesh_entry(ctx, cloud, tx, ty)
    for kw, text in [(dict(nfield=0), 'pgw_gauss_interp_points: nfield must be in [1, 16]'),
                     (dict(nfield=17), 'pgw_gauss_interp_points: nfield must be in [1, 16]'),
                     (dict(cell=np.nextafter(1.0, 0.0)),
                      'pgw_gauss_interp_points: cells must be at least one kernel radius wide (3 x 3 block search)'),
                     (dict(cell=0.0), 'pgw_gauss_interp_points: bad cell grid'),
                     (dict(ntarg=0), 'pgw_gauss_interp_points: bad argument'),
                     (dict(ntarg=2 ** 31),
                      'pgw_gauss_interp_points: ntarg must be below 2^31 (the order of the targets is kept in 32-bit indices)')]:
        with pytest.raises(ValueError) as e:
            _points(ctx, cloud, tx, ty, **kw)
        assert str(e.value) == text
        _assert_same_bits(_points(ctx, cloud, tx, ty), good, 'first call after the error')


# ------------------------------------------------------------------ pgw_ocean_targets
def _mesh_13x20():
    return np.linspace(-90.0, 90.0, 13), np.arange(20) * 18.0


def _host_mesh_coordinates(elat, elon_raw):
    """(tx, ty) of a mesh as gauss_interp_fields forms them on the host: the distinct |lat| x |lon| through
    functions.planar_metres, then the signs."""
    from pgw4era5_amd import functions as F
    elon = F._fold_lon(elon_raw)
    la_u, la_i = np.unique(np.abs(elat), return_inverse=True)
    lo_u, lo_i = np.unique(np.abs(elon), return_inverse=True)
    uu_lat, uu_lon = np.repeat(la_u, len(lo_u)), np.tile(lo_u, len(la_u))
    u_arc, u_lon, _ = F.planar_metres(uu_lat, uu_lon)
    lat_arc = u_arc.reshape(len(la_u), len(lo_u))[:, 0]
    lon_arc = u_lon.reshape(len(la_u), len(lo_u))
    tx = (lat_arc[la_i] * np.sign(elat))[:, None] * np.ones(len(elon))[None, :]
    ty = lon_arc[np.ix_(la_i, lo_i)] * np.sign(elon)[None, :]
    return tx, ty


def _ocean_targets(ctx, lat, lon, land):
    n = lat.size
    d_lat, d_lon = ctx.to_device(np.ascontiguousarray(lat.ravel())), ctx.to_device(np.ascontiguousarray(lon.ravel()))
    d_land = None if land is None else ctx.to_device(np.ascontiguousarray(land.ravel()))
    d_tx, d_ty = ctx.to_device(np.full(n, SENTINEL)), ctx.to_device(np.full(n, SENTINEL))
    ctx._check(ctx.lib.pgw_ocean_targets(ctx.handle, n, d_lat.ptr, d_lon.ptr, None if d_land is None else d_land.ptr, d_tx.ptr,
                                         d_ty.ptr))
    return d_tx.numpy().reshape(lat.shape), d_ty.numpy().reshape(lat.shape)


def test_ocean_targets_give_the_mesh_path_bits(ctx):
    elat, elon = _mesh_13x20()
    assert elat[0] == -90.0 and elat[-1] == 90.0 and elat[6] == 0.0 and 0.0 in elon and 180.0 in elon and (elon > 180.0).sum() == 9
    lat2, lon2 = np.meshgrid(elat, elon, indexing='ij')
    rng = np.random.default_rng(10)
    land = rng.uniform(0.0, 0.69, (13, 20))
    land[rng.uniform(size=(13, 20)) < 0.2] = 0.9
    land[4, 4], land[5, 5], land[12, 0], land[6, 10] = 0.7, np.nan, 1.0, 0.71
    above = land > 0.7
    assert 20 < above.sum() < 100 and not above[4, 4] and not above[5, 5]
    want_x, want_y = _host_mesh_coordinates(elat, elon)
    tx, ty = _ocean_targets(ctx, lat2, lon2, None)
    _assert_same_bits(tx, want_x, 'tx'); _assert_same_bits(ty, want_y, 'ty')
    assert (ty[:, elon > 180.0][1:-1] < 0).all() and (ty[1:-1, 10] > 0).all() and (ty[[0, -1]] == 0).all() and (tx[6] == 0).all()
    tx, ty = _ocean_targets(ctx, lat2, lon2, land)
    np.testing.assert_array_equal(np.isnan(tx), above); np.testing.assert_array_equal(np.isnan(ty), above)
    _assert_same_bits(tx[~above], want_x[~above], 'tx of the ocean targets'); _assert_same_bits(ty[~above], want_y[~above], 'ty')
    # a NaN coordinate is inactive whatever the land fraction; n = 0 is no launch
    la, lo = lat2.copy(), lon2.copy()
    la[3, 3], lo[8, 2] = np.nan, np.nan
    tx, ty = _ocean_targets(ctx, la, lo, None)
    assert np.isnan(tx).sum() == 2 and np.isnan(tx[3, 3]) and np.isnan(ty[3, 3]) and np.isnan(tx[8, 2]) and np.isnan(ty[8, 2])
    ctx._check(ctx.lib.pgw_ocean_targets(ctx.handle, 0, None, None, None, None, None))


# ------------------------------------------------------------------ functions.gauss_interp_points
R_SMALL, S_SMALL = 2.5e6, 4.0


@pytest.fixture(scope='module')
def small():
    """The setup of test_gauss_interp_vs_oracle_small and its mesh-path result."""
    from pgw4era5_amd import functions as F, synthetic
    oc = synthetic.make_ocean_grid_case(nj=18, ni=26, ntime=3, seed=2)
    lat, lon = _mesh_13x20()
    land = (np.random.default_rng(1).uniform(size=(13, 20)) > 0.8).astype(np.float64)
    mesh = F.gauss_interp_fields(land, lat, lon, oc['latitude'], oc['longitude'], list(oc['values']), R_SMALL, S_SMALL)
    mesh.setflags(write=False)
    return dict(oc=oc, lat=lat, lon=lon, land=land, mesh=mesh)


def test_a_mesh_handed_over_as_points_gives_the_mesh_bits(small):
    from pgw4era5_amd import functions as F
    oc, land, mesh = small['oc'], small['land'], small['mesh']
    lat2, lon2 = np.meshgrid(small['lat'], small['lon'], indexing='ij')
    args = (oc['latitude'], oc['longitude'], list(oc['values']), R_SMALL, S_SMALL)
    assert lat2.size == 260 and 0 < (land > 0.7).sum() < 130 and np.isnan(mesh).any() and not np.isnan(mesh).all()
    got = F.gauss_interp_points(land, lat2, lon2, *args)
    assert got.shape == (3, 13, 20) and got.dtype == np.float64
    _assert_same_bits(got, np.asarray(mesh), 'the meshgrid as a (13, 20) array')
    rng = np.random.default_rng(11)
    p = rng.permutation(260)
    got = F.gauss_interp_points(land.ravel()[p], lat2.ravel()[p], lon2.ravel()[p], *args)
    assert got.shape == (3, 260)
    _assert_same_bits(got, np.ascontiguousarray(mesh.reshape(3, 260)[:, p]), 'flattened and permuted')
    q = np.concatenate([p, p[:40]])
    got = F.gauss_interp_points(land.ravel()[q], lat2.ravel()[q], lon2.ravel()[q], *args)
    _assert_same_bits(got, np.ascontiguousarray(mesh.reshape(3, 260)[:, q]), 'with 40 targets repeated')
    got = F.gauss_interp_points(None, lat2, lon2, *args)            # no land field: the mesh path with no land
    _assert_same_bits(got, F.gauss_interp_fields(np.zeros((13, 20)), small['lat'], small['lon'], *args), 'land_fr = None')


@pytest.fixture(scope='module')
def scattered():
    """A rotated-pole grid (5 x 7) plus a cell list of 300 points over the globe, as one cell list of 335 targets."""
    from pgw4era5_amd import synthetic
    rng = np.random.default_rng(12)
    _, _, rlat2, rlon2 = synthetic.rotated_pole_grid(5, 7)
    lat = np.concatenate([[90.0, -90.0, 30.0, -40.0, 12.0, 55.0], rng.uniform(-90.0, 90.0, 294)])
    lon = np.concatenate([[10.0, -50.0, 180.0, -180.0, 0.0, 359.5], rng.uniform(-180.0, 360.0, 294)])
    folded = np.where(lon > 180.0, lon - 360.0, lon)
    bad = (np.abs(lat) < 2.0) & (np.abs(folded) > 170.0) & (np.abs(folded) < 180.0)
    lat[bad] += 5.0                                                 # the oracle's geodesic inverse does not converge there
    lat, lon = np.concatenate([rlat2.ravel(), lat]), np.concatenate([rlon2.ravel(), lon])
    folded = np.where(lon > 180.0, lon - 360.0, lon)
    assert not ((np.abs(lat) < 2.0) & (np.abs(folded) > 170.0) & (np.abs(folded) < 180.0)).any()
    assert len(lat) == 335 and (lon > 180.0).sum() > 50 and (lon < 0.0).sum() > 50
    land = np.where(rng.uniform(size=335) < 0.2, 0.9, 0.1)
    assert 40 < (land > 0.7).sum() < 100
    return lat, lon, land


def _oracle_points(lat, lon, land, oc, values):
    return np.array([O.nan_ignoring_interp(np.array([[land[i]]]), lat[i:i + 1], lon[i:i + 1], oc['latitude'], oc['longitude'],
                                           values, R_SMALL, S_SMALL)[0, 0] for i in range(len(lat))])


@pytest.fixture(scope='module')
def scattered_result(small, scattered):
    from pgw4era5_amd import functions as F
    oc = small['oc']
    lat, lon, land = scattered
    got = F.gauss_interp_points(land, lat, lon, oc['latitude'], oc['longitude'], list(oc['values']), R_SMALL, S_SMALL)
    got.setflags(write=False)
    return got


def test_points_against_the_oracle(small, scattered, scattered_result):
    oc, got = small['oc'], scattered_result
    lat, lon, land = scattered
    assert got.shape == (3, 335)
    want = _oracle_points(lat, lon, land, oc, oc['values'][0])
    np.testing.assert_allclose(got[0], want, rtol=1e-10, atol=0, equal_nan=True)
    n_land = int((land > 0.7).sum())
    assert np.isnan(want).sum() >= n_land > 0 and np.isfinite(want).sum() > 0.6 * len(want)
    assert np.isnan(got[:, land > 0.7]).all()


def test_points_month_with_its_own_nan_patch(small, scattered, scattered_result):
    """That month's cloud loses the points (it matches the oracle), the other months keep their bits."""
    from pgw4era5_amd import functions as F
    oc, got = small['oc'], scattered_result
    lat, lon, land = scattered
    v2 = oc['values'].copy()
    v2[1, 3:9, 5:15] = np.nan
    got2 = F.gauss_interp_points(land, lat, lon, oc['latitude'], oc['longitude'], list(v2), R_SMALL, S_SMALL)
    _assert_same_bits(got2[0], np.asarray(got[0]), 'month 0'); _assert_same_bits(got2[2], np.asarray(got[2]), 'month 2')
    want = _oracle_points(lat, lon, land, oc, v2[1])
    np.testing.assert_allclose(got2[1], want, rtol=1e-10, atol=0, equal_nan=True)
    assert np.nanmax(np.abs(got2[1] - got[1])) > 1e-6


def test_nan_ignoring_interp_with_labelled_2d_coordinates(small):
    from pgw4era5_amd import functions as F, ncio, synthetic
    oc = small['oc']
    _, _, lat2, lon2 = synthetic.rotated_pole_grid(5, 7)
    land = (np.random.default_rng(13).uniform(size=(5, 7)) > 0.8).astype(np.float64)
    da_land = ncio.Field(land, ('rlat', 'rlon'), {'lat': lat2, 'lon': lon2})
    da_delta = ncio.Field(oc['values'][1], ('j', 'i'), {'latitude': oc['latitude'], 'longitude': oc['longitude']})
    got = F.nan_ignoring_interp(da_land, da_delta, R_SMALL, S_SMALL)
    want = F.gauss_interp_points(land, lat2, lon2, oc['latitude'], oc['longitude'], [oc['values'][1]], R_SMALL, S_SMALL)[0]
    assert got.shape == (5, 7) and 0 < np.isnan(got).sum() < 35
    _assert_same_bits(got, want)
    # a mesh stays on the mesh path
    lat, lon = small['lat'], small['lon']
    got = F.nan_ignoring_interp(ncio.Field(small['land'], ('lat', 'lon'), {'lat': lat, 'lon': lon}), da_delta, R_SMALL, S_SMALL)
    _assert_same_bits(got, np.ascontiguousarray(small['mesh'][1]))


# ------------------------------------------------------------------ step_02 regridding onto an extpar file
@pytest.mark.parametrize('land_time_axis', [False, True])
def test_step02_regridding_onto_an_extpar_file(tmp_path, land_time_axis):
    from pgw4era5_amd import functions as F, ncio, settings as S, step_02_preproc_deltas as s2, synthetic
    inp, out, ext = tmp_path / 'gcm', tmp_path / 'regridded', str(tmp_path / 'extpar.nc')
    synthetic.write_gcm_files(str(inp), ocean=(30, 44))
    synthetic.make_extpar(ext)
    target = ncio.open_dataset(ext, decode_times=False)
    land = np.asarray(target['FR_LAND'].values, dtype=np.float64)
    lat2, lon2 = np.asarray(target['lat'].values, dtype=np.float64), np.asarray(target['lon'].values, dtype=np.float64)
    assert target['FR_LAND'].dims == ('rlat', 'rlon') and land.shape == lat2.shape == (7, 9) and 0 < (land > 0.7).sum() < 63
    if land_time_axis:                                             # the reference's layout: FR_LAND[0, :, :]
        target['time'] = ncio.Field(np.array([0.0]), ('time',))
        target['FR_LAND'] = ncio.Field(target['FR_LAND'].values[None], ('time', 'rlat', 'rlon'), attrs=target['FR_LAND'].attrs)
        ext = str(tmp_path / 'extpar_time.nc')
        ncio.to_netcdf(target, ext)
        assert ncio.open_dataset(ext, decode_times=False)['FR_LAND'].shape == (1, 7, 9)
    done = s2.main(['regridding', '-i', str(inp), '-o', str(out), '-e', ext, '-v', 'tos,siconc,ts'])
    assert len(done) == 6
    for var in ('tos', 'siconc'):
        for base in ('%s_delta.nc', '%s_historical.nc'):
            src = ncio.open_dataset(str(inp / (base % var)))
            res = ncio.open_dataset(str(out / (base % var)))
            assert res[var].dims == ('time', 'rlat', 'rlon') and res[var].shape == (12, 7, 9)
            assert res['lat'].dims == res['lon'].dims == ('rlat', 'rlon')
            np.testing.assert_array_equal(res['lat'].values, lat2); np.testing.assert_array_equal(res['lon'].values, lon2)
            np.testing.assert_array_equal(res['time'].values, src['time'].values)
            assert res.attrs['description'] == var + ' on ERA5 grid'
            want = F.gauss_interp_points(land, lat2, lon2, src['latitude'].values, src['longitude'].values,
                                         [src[var].values[m] for m in range(12)], S.nan_interp_kernel_radius, S.nan_interp_sharpness)
            _assert_same_bits(np.asarray(res[var].values, dtype=np.float64), want, var)
            assert np.isnan(res[var].values[:, land > 0.7]).all() and not np.isnan(res[var].values).all()
    ts = ncio.open_dataset(str(out / 'ts_delta.nc'))
    want = F.regrid_lat_lon(ncio.open_dataset(str(inp / 'ts_delta.nc')), ncio.open_dataset(ext, decode_times=False), 'ts')
    assert ts['ts'].dims == ('time', 'rlat', 'rlon') and not np.isnan(ts['ts'].values).any()
    _assert_same_bits(np.ascontiguousarray(ts['ts'].values), np.ascontiguousarray(want['ts'].values), 'ts')
